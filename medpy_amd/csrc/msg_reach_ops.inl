/*
 * msg_reach_ops.inl -- the other minimum cuts of a graph on the sparse-graph solver: node operations and schedule of the flood
 * behind msg_cut_sets / msg_cut_sets_tol.  The counterpart, over CSR arcs, of what mgc_reach_ops.inl and
 * mgc_reach_tol_ops.inl do over tile masks for the voxel solver.
 *
 * Starting point: a converged msg_solve (msg_node_ops.inl).  No flow is in flight then -- every `delta` slot is 0.0, every node
 * with excess > 0 stands at MSG_HINF, every node with sink > 0 has label 1 and no excess -- so rcap / excess / sink are a maximum
 * PREFLOW.  The set reachable from {excess > 0} in a preflow's residual graph is the source-reachable set of the maximum flow the
 * preflow decomposes into: the argument of DESIGN 13 carries over word for word (it never uses the lattice), see there for the proof.
 *
 * The rule (DESIGN 13b's, with "arc pair at a voxel" read as "CSR arc a and rev[a]"):
 *   pair(a)  = cap0[a] + cap0[rev[a]]          -- the capacities as built, which this solver keeps
 *   scale(v) = the largest pair(a) over the row of v, never below 0; 0 for a node without arcs
 *   arc u -> v is open      iff rcap > 0 && rcap > tol * max(scale(u), scale(v))
 *   v is a source seed      iff excess(v) > 0 && excess(v) > tol * max(|tr(v)|, scale(v))
 *   v is a sink seed        iff sink(v)   > 0 && sink(v)   > tol * max(|tr(v)|, scale(v))
 * with tr the merged t-link the handle holds (0 without one).  from_source = what the source seeds reach along open arcs, to_sink =
 * what reaches a sink seed along them, ambiguous = neither.  Without a tolerance (use_tol == 0) an arc is open iff rcap > 0, seeds are
 * excess > 0, and to_sink is read off the exact labels (height < MSG_HINF): no scale, no backward flood.  tol == 0 multiplies
 * nothing (msg_reach_threshold), so it gives the same sets by the longer way.
 *
 * Single source for the HIP kernels (msg_sparse.hip) and the host simulator of the CPU tests
 * (tests/hostsim/hostsim_sparse_reach.cpp, tests/hostsim/sparse_reach_main.cpp).
 */
#ifndef MSG_REACH_OPS_INL
#define MSG_REACH_OPS_INL

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "msg_node_ops.inl"

struct MsgReach {
    int64_t nodes, arcs;
    const int64_t* row;     /* [nodes + 1]                                                                 */
    const int32_t* head;    /* [arcs]                                                                      */
    const int64_t* rev;     /* [arcs]                                                                      */
    const double* rcap;     /* [arcs] residual capacities of the converged solve                           */
    const double* cap0;     /* [arcs] capacities as built                                                  */
    const double* excess;   /* [nodes]                                                                     */
    const double* sink;     /* [nodes]                                                                     */
    const double* tr;       /* [nodes] merged t-links, or NULL (all 0)                                     */
    const int32_t* height;  /* [nodes] exact labels                                                        */
    int use_tol;            /* 0: msg_cut_sets, 1: msg_cut_sets_tol                                        */
    double tol;
    double* scale;          /* [nodes] (use_tol only)                                                      */
    uint8_t* open;          /* [arcs] bit 0: arc a is open (v -> head), bit 1: rev[a] is open (head -> v)  */
    uint8_t* mark[2];       /* [nodes] 0 / 1: reached by the forward flood [0] / the backward flood [1]    */
    uint8_t* to_sink;       /* [nodes] read-out planes; from_source is mark[0] itself                      */
    uint8_t* ambiguous;
    uint8_t* not_to_sink;   /* the label plane k_msg_cut_value takes for sink_cut                          */
    int32_t* count;         /* the solver's four counters: 2 = a forward pass marked a node, 3 = a backward pass did */
};

/* what msg_reach reports */
struct MsgReachInfo {
    int64_t from_source, to_sink, ambiguous;
    int64_t forward_passes, forward_seeds, backward_passes, backward_seeds;
    int64_t arcs_closed, tlinks_closed; /* rcap > 0 / excess > 0 or sink > 0 that the threshold closed */
    int64_t tol_path;
    double scale_max;
};

/* slots of the tallies a device adds up while the kernels run (read once, at the end) */
enum {
    MSG_REACH_T_FROM = 0, MSG_REACH_T_TO = 1, MSG_REACH_T_AMB = 2, MSG_REACH_T_SEED_F = 3, MSG_REACH_T_SEED_B = 4, MSG_REACH_T_ARCS_CLOSED = 5,
    MSG_REACH_T_TLINKS_CLOSED = 6, MSG_REACH_T_SCALE_MAX = 7 /* the bit pattern of a double >= 0: ordered like the number */, MSG_REACH_NTALLY = 8
};

/* tol * s; tol == 0 multiplies nothing, so an infinite scale cannot make a NaN of it */
MSG_HD double msg_reach_threshold(double tol, double s) { return tol > 0.0 ? tol * s : 0.0; }

MSG_HD double msg_reach_scale_node(const MsgReach& R, int64_t v)
{
    double s = 0.0;
    for (int64_t a = R.row[v]; a < R.row[v + 1]; ++a) {
        const double p = R.cap0[a] + R.cap0[R.rev[a]];
        if (p > s) s = p;
    }
    R.scale[v] = s;
    return s;
}

/* the open byte of every arc of v's own row; returns how many of them have rcap > 0 and were closed by the threshold (bit 0 only:
 * every arc is the bit 0 of exactly one row) */
MSG_HD int64_t msg_reach_open_node(const MsgReach& R, int64_t v)
{
    int64_t closed = 0;
    const double sv = R.use_tol ? R.scale[v] : 0.0;
    for (int64_t a = R.row[v]; a < R.row[v + 1]; ++a) {
        double thr = 0.0;
        if (R.use_tol) {
            const double sw = R.scale[R.head[a]];
            thr = msg_reach_threshold(R.tol, sv > sw ? sv : sw);
        }
        const double r = R.rcap[a], rr = R.rcap[R.rev[a]];
        const bool o0 = r > 0.0 && r > thr, o1 = rr > 0.0 && rr > thr;
        R.open[a] = (uint8_t)((o0 ? 1 : 0) | (o1 ? 2 : 0));
        if (r > 0.0 && !o0) closed++;
    }
    return closed;
}

/* start of a flood: the mark of v.  Returns 1 for a seed, 2 for a t-link residual > 0 that the threshold closed, else 0 */
template <bool BACK>
MSG_HD int msg_reach_seed_node(const MsgReach& R, int64_t v)
{
    const double x = BACK ? R.sink[v] : R.excess[v];
    bool seed = false;
    if (x > 0.0) {
        double thr = 0.0;
        if (R.use_tol) {
            const double t = R.tr ? fabs(R.tr[v]) : 0.0, s = R.scale[v];
            thr = msg_reach_threshold(R.tol, t > s ? t : s);
        }
        seed = x > thr;
    }
    R.mark[BACK ? 1 : 0][v] = seed ? 1 : 0;
    return x > 0.0 ? (seed ? 1 : 2) : 0;
}

/* One step of a flood at node v; returns true when v got its mark.  Forward: v is reached when some marked neighbour has its arc
 * INTO v open (bit 1 of v's own arc); backward: when v's own arc to a marked neighbour is open (bit 0).
 * Any order, any interleaving: marks only go 0 -> 1, and a node only ever writes its own.  A neighbour's mark read as a stale 0
 * (another workgroup set it in this very launch) is read again in the next pass -- the setter has raised the counter, so there is
 * one: it costs a pass, never a node.  The marks at the fixpoint are the reachable set whatever the order was. */
template <bool BACK>
MSG_HD bool msg_reach_pass_node(const MsgReach& R, int64_t v)
{
    uint8_t* const m = R.mark[BACK ? 1 : 0];
    if (m[v]) return false;
    const uint8_t bit = BACK ? 1 : 2;
    for (int64_t a = R.row[v]; a < R.row[v + 1]; ++a)
        if ((R.open[a] & bit) && m[R.head[a]]) {
            m[v] = 1;
            return true;
        }
    return false;
}

/* the planes of v; returns bit 0: from_source, bit 1: to_sink, bit 2: ambiguous */
MSG_HD int msg_reach_readout_node(const MsgReach& R, int64_t v)
{
    const int f = R.mark[0][v] ? 1 : 0;
    const int t = R.use_tol ? (R.mark[1][v] ? 1 : 0) : (R.height[v] < MSG_HINF ? 1 : 0);
    const int amb = (f | t) ? 0 : 1;
    R.to_sink[v] = (uint8_t)t;
    R.ambiguous[v] = (uint8_t)amb;
    R.not_to_sink[v] = (uint8_t)(1 - t);
    return f | (t << 1) | (amb << 2);
}

/* schedule shared by the library and the simulator: Dev provides reach_begin() (tallies to 0), reach_scale(), reach_open(),
 * reach_seed(back), reach_pass(back), reach_readout(), zero_count(i), read_counts(int[4]), read_tally(uint64[MSG_REACH_NTALLY]),
 * which waits for everything before it, and phase_done(k), a time stamp behind phase k (MSG_REACH_PHASE_*; the simulator keeps none).
 * Passes run in stretches of 8 between two looks, as the relabel loop of msg_solve does. */
enum { MSG_REACH_PHASE_START = 0, MSG_REACH_PHASE_SCALE = 1, MSG_REACH_PHASE_OPEN = 2, MSG_REACH_PHASE_FORWARD = 3, MSG_REACH_PHASE_BACKWARD = 4,
       MSG_REACH_PHASE_READOUT = 5, MSG_REACH_NPHASE = 6 };

template <class Dev>
void msg_reach(Dev& dev, bool use_tol, MsgReachInfo& info)
{
    info = MsgReachInfo();
    info.tol_path = use_tol ? 1 : 0;
    int cnt[4];
    dev.reach_begin();
    dev.phase_done(MSG_REACH_PHASE_START);
    if (use_tol) dev.reach_scale();
    dev.phase_done(MSG_REACH_PHASE_SCALE);
    dev.reach_open();
    dev.phase_done(MSG_REACH_PHASE_OPEN);
    for (int back = 0; back < (use_tol ? 2 : 1); ++back) {
        dev.reach_seed(back);
        int64_t& passes = back ? info.backward_passes : info.forward_passes;
        for (;;) {
            dev.zero_count(2 + back);
            for (int b = 0; b < 8; ++b) { dev.reach_pass(back); passes++; }
            dev.read_counts(cnt);
            if (!cnt[2 + back]) break;
        }
        dev.phase_done(back ? MSG_REACH_PHASE_BACKWARD : MSG_REACH_PHASE_FORWARD);
    }
    if (!use_tol) dev.phase_done(MSG_REACH_PHASE_BACKWARD);
    dev.reach_readout();
    unsigned long long t[MSG_REACH_NTALLY];
    dev.read_tally(t);
    info.from_source = (int64_t)t[MSG_REACH_T_FROM]; info.to_sink = (int64_t)t[MSG_REACH_T_TO]; info.ambiguous = (int64_t)t[MSG_REACH_T_AMB];
    info.forward_seeds = (int64_t)t[MSG_REACH_T_SEED_F]; info.backward_seeds = (int64_t)t[MSG_REACH_T_SEED_B];
    info.arcs_closed = (int64_t)t[MSG_REACH_T_ARCS_CLOSED]; info.tlinks_closed = (int64_t)t[MSG_REACH_T_TLINKS_CLOSED];
    double smax = 0.0;
    memcpy(&smax, &t[MSG_REACH_T_SCALE_MAX], sizeof(smax));
    info.scale_max = smax;
}

#endif /* MSG_REACH_OPS_INL */
