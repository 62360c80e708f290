/*
 * hostsim_sparse_reach.cpp -- TEST ONLY.  msg_cut_sets / msg_cut_sets_tol of the sparse-graph solver on the host: the node operations
 * and the schedule of medpy_amd/csrc/msg_reach_ops.inl (the same source the k_msg_reach_* kernels compile) after the solve of
 * msg_node_ops.inl, so the CPU test tier can check the sets against the exact oracle without a GPU.  The CSR assembly is that of
 * hostsim_sparse.cpp.  One entry: build, solve, then one flood per entry of tols[] (a negative entry = the call without a tolerance).
 */
#include <algorithm>
#include <numeric>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../medpy_amd/csrc/msg_reach_ops.inl"

namespace {

struct HostSparse {
    MsgCsr G;
    std::vector<int64_t> row, rev;
    std::vector<int32_t> head, tail, height;
    std::vector<double> rcap, cap0, delta, excess, sink;
    int32_t count[4];

    void relabel_init() { for (int64_t u = 0; u < G.nodes; ++u) msg_relabel_init_node(G, u); }
    void relabel_pass() { for (int64_t u = 0; u < G.nodes; ++u) if (msg_relabel_relax_node(G, u)) count[1] = 1; }
    void push() { for (int64_t u = 0; u < G.nodes; ++u) msg_push_node(G, u); }
    void gather() { for (int64_t u = 0; u < G.nodes; ++u) if (msg_gather_node(G, u)) count[0] = 1; }
    void count_active() { for (int64_t u = 0; u < G.nodes; ++u) if (msg_active_node(G, u)) count[0] = 1; }
    void zero_count(int i) { count[i] = 0; }
    void read_counts(int* out) { memcpy(out, count, sizeof(count)); }

    /* the capacity of the cut around the nodes with labels[u] != 0, from the capacities as built (k_msg_cut_value) */
    double cut_value(const double* tr, const uint8_t* labels) const
    {
        double cut = 0.0;
        for (int64_t u = 0; u < G.nodes; ++u) {
            const double t = tr ? tr[u] : 0.0;
            if (labels[u]) {
                if (t < 0) cut += -t;
                for (int64_t a = row[u]; a < row[u + 1]; ++a)
                    if (!labels[head[a]]) cut += cap0[a];
            } else if (t > 0) {
                cut += t;
            }
        }
        return cut;
    }
};

/* the device of msg_reach: every "kernel" is a loop over the nodes */
struct HostReach {
    MsgReach R;
    int32_t* count;
    unsigned long long tally[MSG_REACH_NTALLY];
    std::vector<double> scale;
    std::vector<uint8_t> open, mark0, mark1, to, amb, nts;

    void reach_begin() { memset(tally, 0, sizeof(tally)); }
    void phase_done(int) {}
    void reach_scale()
    {
        double m = 0.0;
        for (int64_t v = 0; v < R.nodes; ++v) { const double s = msg_reach_scale_node(R, v); if (s > m) m = s; }
        memcpy(&tally[MSG_REACH_T_SCALE_MAX], &m, sizeof(m));
    }
    void reach_open() { for (int64_t v = 0; v < R.nodes; ++v) tally[MSG_REACH_T_ARCS_CLOSED] += (unsigned long long)msg_reach_open_node(R, v); }
    void reach_seed(int back)
    {
        for (int64_t v = 0; v < R.nodes; ++v) {
            const int k = back ? msg_reach_seed_node<true>(R, v) : msg_reach_seed_node<false>(R, v);
            if (k == 1) tally[back ? MSG_REACH_T_SEED_B : MSG_REACH_T_SEED_F]++;
            if (k == 2) tally[MSG_REACH_T_TLINKS_CLOSED]++;
        }
    }
    void reach_pass(int back)
    {
        for (int64_t v = 0; v < R.nodes; ++v)
            if (back ? msg_reach_pass_node<true>(R, v) : msg_reach_pass_node<false>(R, v)) count[2 + back] = 1;
    }
    void reach_readout()
    {
        for (int64_t v = 0; v < R.nodes; ++v) {
            const int k = msg_reach_readout_node(R, v);
            tally[MSG_REACH_T_FROM] += k & 1;
            tally[MSG_REACH_T_TO] += (k >> 1) & 1;
            tally[MSG_REACH_T_AMB] += (k >> 2) & 1;
        }
    }
    void zero_count(int i) { count[i] = 0; }
    void read_counts(int* out) { memcpy(out, count, 4 * sizeof(int32_t)); }
    void read_tally(unsigned long long* out) { memcpy(out, tally, sizeof(tally)); }
};

} // namespace

/* tols[n_tol]: a negative entry stands for msg_cut_sets, any other for msg_cut_sets_tol.  labels_out[nodes], *flow_out: the solve.
 * sets_out[n_tol][3][nodes]: from_source, to_sink, ambiguous; info_out[n_tol][16] / vals_out[n_tol][4]: what msg_get_cut_sets_info
 * reports.  *arcs_out, tail_out / head_out / rcap_out / cap0_out[2 * n_edges], excess_out / sink_out[nodes]: the residual graph the
 * floods ran on (they change none of it: the function checks that and returns 2 otherwise).  Returns 1 when the solve did not converge. */
extern "C" int hostsim_sparse_reach(int64_t nodes, int64_t n_edges, const int64_t* ei, const int64_t* ej, const double* ecap, const double* erev,
                                    const double* tr, double flow_const, int rounds_per_relabel, int n_tol, const double* tols, uint8_t* labels_out,
                                    double* flow_out, uint8_t* sets_out, int64_t* info_out, double* vals_out, int64_t* arcs_out, int32_t* tail_out,
                                    int32_t* head_out, double* rcap_out, double* cap0_out, double* excess_out, double* sink_out)
{
    HostSparse d;
    const int64_t n2 = 2 * n_edges;
    std::vector<uint64_t> key((size_t)n2);
    std::vector<uint32_t> idx((size_t)n2);
    for (int64_t e = 0; e < n_edges; ++e) {
        key[2 * e] = ((uint64_t)ei[e] << 32) | (uint64_t)ej[e];
        key[2 * e + 1] = ((uint64_t)ej[e] << 32) | (uint64_t)ei[e];
    }
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    for (int64_t k = 0; k < n2;) {
        const uint64_t kk = key[idx[k]];
        double s = 0.0;
        int64_t m = k;
        for (; m < n2 && key[idx[m]] == kk; ++m) {
            const uint32_t a = idx[m];
            s += (a & 1) ? erev[a >> 1] : ecap[a >> 1];
        }
        d.head.push_back((int32_t)(kk & 0xffffffffu));
        d.tail.push_back((int32_t)(kk >> 32));
        d.cap0.push_back(s);
        k = m;
    }
    const int64_t A = (int64_t)d.head.size();
    d.row.assign((size_t)nodes + 1, 0);
    for (int64_t a = 0; a < A; ++a) d.row[(size_t)d.tail[a] + 1]++;
    for (int64_t u = 0; u < nodes; ++u) d.row[u + 1] += d.row[u];
    d.rev.assign((size_t)A, 0);
    for (int64_t a = 0; a < A; ++a) {
        const int32_t v = d.head[a], u = d.tail[a];
        const auto b = d.head.begin() + d.row[v], e = d.head.begin() + d.row[v + 1];
        d.rev[a] = std::lower_bound(b, e, u) - d.head.begin();
    }
    d.rcap = d.cap0;
    d.delta.assign((size_t)A, 0.0);
    d.excess.assign((size_t)nodes, 0.0);
    d.sink.assign((size_t)nodes, 0.0);
    d.height.assign((size_t)nodes, MSG_HINF);
    for (int64_t u = 0; u < nodes; ++u) {
        const double t = tr ? tr[u] : 0.0;
        d.excess[u] = t > 0 ? t : 0.0;
        d.sink[u] = t < 0 ? -t : 0.0;
    }
    memset(d.count, 0, sizeof(d.count));
    MsgCsr& G = d.G;
    G.nodes = nodes; G.arcs = A; G.row = d.row.data(); G.head = d.head.data(); G.rev = d.rev.data(); G.rcap = d.rcap.data();
    G.delta = d.delta.data(); G.excess = d.excess.data(); G.sink = d.sink.data(); G.height = d.height.data(); G.count = d.count;
    MsgSolveStats st;
    const int rc = msg_solve(d, rounds_per_relabel > 0 ? rounds_per_relabel : 64, (int64_t)1 << 40, st);
    for (int64_t u = 0; u < nodes; ++u) labels_out[u] = d.height[u] < MSG_HINF ? 0 : 1;
    const double flow = flow_const + d.cut_value(tr, labels_out);
    *flow_out = flow;
    *arcs_out = A;
    for (int64_t a = 0; a < A; ++a) { tail_out[a] = d.tail[a]; head_out[a] = d.head[a]; rcap_out[a] = d.rcap[a]; cap0_out[a] = d.cap0[a]; }
    for (int64_t u = 0; u < nodes; ++u) { excess_out[u] = d.excess[u]; sink_out[u] = d.sink[u]; }
    if (rc) return 1;
    for (int64_t a = 0; a < A; ++a)
        if (d.delta[a] != 0.0) return 3; /* flow in flight after a converged solve: the starting point of the flood does not hold */
    const std::vector<double> rcap_before = d.rcap, excess_before = d.excess, sink_before = d.sink;
    const std::vector<int32_t> height_before = d.height;

    for (int k = 0; k < n_tol; ++k) {
        const bool use_tol = !(tols[k] < 0.0);
        HostReach dev;
        dev.count = d.count;
        dev.scale.assign((size_t)nodes, 0.0);
        dev.open.assign((size_t)(A ? A : 1), 0);
        dev.mark0.assign((size_t)nodes, 0); dev.mark1.assign((size_t)nodes, 0);
        dev.to.assign((size_t)nodes, 0); dev.amb.assign((size_t)nodes, 0); dev.nts.assign((size_t)nodes, 0);
        MsgReach& R = dev.R;
        R.nodes = nodes; R.arcs = A; R.row = d.row.data(); R.head = d.head.data(); R.rev = d.rev.data(); R.rcap = d.rcap.data(); R.cap0 = d.cap0.data();
        R.excess = d.excess.data(); R.sink = d.sink.data(); R.tr = tr; R.height = d.height.data();
        R.use_tol = use_tol ? 1 : 0; R.tol = use_tol ? tols[k] : 0.0;
        R.scale = dev.scale.data(); R.open = dev.open.data(); R.mark[0] = dev.mark0.data(); R.mark[1] = dev.mark1.data();
        R.to_sink = dev.to.data(); R.ambiguous = dev.amb.data(); R.not_to_sink = dev.nts.data(); R.count = d.count;
        MsgReachInfo info;
        msg_reach(dev, use_tol, info);
        uint8_t* out = sets_out + (size_t)k * 3 * (size_t)nodes;
        memcpy(out, dev.mark0.data(), (size_t)nodes);
        memcpy(out + nodes, dev.to.data(), (size_t)nodes);
        memcpy(out + 2 * nodes, dev.amb.data(), (size_t)nodes);
        int64_t* o = info_out + 16 * k;
        memset(o, 0, 16 * sizeof(int64_t));
        o[0] = info.from_source; o[1] = info.to_sink; o[2] = info.ambiguous; o[3] = info.forward_passes; o[4] = info.forward_seeds;
        o[5] = info.backward_passes; o[6] = info.backward_seeds; o[7] = info.arcs_closed; o[8] = info.tlinks_closed; o[9] = info.tol_path;
        double* v = vals_out + 4 * k;
        v[0] = use_tol ? tols[k] : -1.0;
        v[1] = flow_const + d.cut_value(tr, dev.mark0.data());
        v[2] = use_tol ? flow_const + d.cut_value(tr, dev.nts.data()) : flow;
        v[3] = info.scale_max;
    }
    if (d.rcap != rcap_before || d.excess != excess_before || d.sink != sink_before || d.height != height_before) return 2;
    return 0;
}
