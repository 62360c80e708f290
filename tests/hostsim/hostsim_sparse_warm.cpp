/*
 * hostsim_sparse_warm.cpp -- TEST ONLY.  The warm re-solve of the sparse-graph solver on the host: the node operations, the
 * schedule and the t-link fold of medpy_amd/csrc/msg_node_ops.inl (the same source the k_msg_* kernels compile), so the CPU test
 * tier can check msg_update_tweights + msg_maxflow against the BK oracle without a GPU.  One entry: build the CSR residual graph
 * (as hostsim_sparse.cpp does), solve, fold a list of new merged t-links into the resident preflow with msg_fold_tlink_node,
 * solve again from that state; labels and cut of both solves and the residual arrays around the fold come back.
 */
#include <algorithm>
#include <numeric>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../medpy_amd/csrc/msg_node_ops.inl"

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

    /* labels = what_segment, cut = the capacity of the cut from the capacities as built (k_msg_labels / k_msg_cut_value) */
    double read_out(const double* tr, uint8_t* labels) const
    {
        double cut = 0.0;
        for (int64_t u = 0; u < G.nodes; ++u) labels[u] = height[u] < MSG_HINF ? 0 : 1;
        for (int64_t u = 0; u < G.nodes; ++u) {
            const double t = tr[u];
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

} // namespace

/* tr[nodes]: the merged t-links, in: of the first solve, out: after the fold.  ids[n_list] / tr_new[n_list]: the update.
 * labels_out[2 * nodes], cut_out[2]: first and second solve.  row_out[nodes + 1], cap0_out / rcap_out[2 * n_edges]: the CSR, its
 * capacities as built and the residuals after the first solve (the fold leaves them alone).  state_out[4 * nodes]: excess and sink
 * before the fold, excess and sink after it.  stats_out[3]: arcs, rounds of the first solve, rounds of the second. */
extern "C" int hostsim_sparse_warm(int64_t nodes, int64_t n_edges, const int64_t* ei, const int64_t* ej, const double* ecap, const double* erev,
                                   double* tr, int64_t n_list, const int64_t* ids, const double* tr_new, int rounds_per_relabel,
                                   uint8_t* labels_out, double* cut_out, int64_t* row_out, double* cap0_out, double* rcap_out, double* state_out,
                                   int64_t* stats_out)
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
        d.excess[u] = tr[u] > 0 ? tr[u] : 0.0;
        d.sink[u] = tr[u] < 0 ? -tr[u] : 0.0;
    }
    memset(d.count, 0, sizeof(d.count));
    MsgCsr& G = d.G;
    G.nodes = nodes; G.arcs = A; G.row = d.row.data(); G.head = d.head.data(); G.rev = d.rev.data(); G.rcap = d.rcap.data();
    G.delta = d.delta.data(); G.excess = d.excess.data(); G.sink = d.sink.data(); G.height = d.height.data(); G.count = d.count;
    const int rpr = rounds_per_relabel > 0 ? rounds_per_relabel : 64;
    MsgSolveStats st0, st1;
    int rc = msg_solve(d, rpr, (int64_t)1 << 40, st0);
    cut_out[0] = d.read_out(tr, labels_out);
    memcpy(row_out, d.row.data(), (size_t)(nodes + 1) * sizeof(int64_t));
    if (A) memcpy(cap0_out, d.cap0.data(), (size_t)A * sizeof(double));
    if (A) memcpy(rcap_out, d.rcap.data(), (size_t)A * sizeof(double));
    memcpy(state_out, d.excess.data(), (size_t)nodes * sizeof(double));
    memcpy(state_out + nodes, d.sink.data(), (size_t)nodes * sizeof(double));
    /* msg_update_tweights on a finished solve: one node function per list entry, arcs untouched */
    for (int64_t k = 0; k < n_list; ++k) msg_fold_tlink_node(G, tr, ids[k], tr_new[k]);
    memcpy(state_out + 2 * nodes, d.excess.data(), (size_t)nodes * sizeof(double));
    memcpy(state_out + 3 * nodes, d.sink.data(), (size_t)nodes * sizeof(double));
    /* msg_maxflow on the warm handle: no build, the schedule goes on from the resident state */
    rc |= msg_solve(d, rpr, (int64_t)1 << 40, st1);
    cut_out[1] = d.read_out(tr, labels_out + nodes);
    stats_out[0] = A; stats_out[1] = st0.rounds; stats_out[2] = st1.rounds;
    return rc;
}
