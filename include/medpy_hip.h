/*
 * medpy_hip.h -- C ABI of libmedpyhip.so: MI355X (gfx950) voxel graph-cut.
 *
 * This is the drop-in boundary for the hot path
 *     medpy.graphcut.graph_from_voxels  (reference medpy/graphcut/generate.py:33-174)
 *   + medpy.graphcut.energy_voxel.*     (reference medpy/graphcut/energy_voxel.py:33-664)
 *   + maxflow.GraphDouble               (reference lib/maxflow/src/wrapper.cpp:59-89 binding of
 *                                        lib/maxflow/src/graph.h / maxflow.cpp)
 * Plain C types only; a handle owns all device memory; every entry point returns an
 * status code (never exit()s, unlike graph.cpp:22,71,95).  The Python host layer
 * (medpy_amd/graphcut) binds these with ctypes and presents the reference's API;
 * INTEGRATION.md shows the binding a MedPy maintainer would add.
 *
 * Node ids are C-order flat indices of the logical array shape, as in the reference
 * (energy_voxel.py:667-677, generate.py:170-172).  All host arrays handed over must be
 * C-contiguous; they are copied into HBM inside the call and may be freed on return.
 */
#ifndef MEDPY_HIP_H
#define MEDPY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgc_graph* mgc_handle;

typedef enum mgc_status {
    MGC_OK = 0,
    MGC_ERR_INVALID = 1,     /* bad argument (shape, dtype, id out of range ...)          */
    MGC_ERR_NO_DEVICE = 2,   /* no usable gfx950 device: the library never falls back     */
    MGC_ERR_HIP = 3,         /* a HIP runtime call failed; see mgc_last_error             */
    MGC_ERR_OOM = 4,
    MGC_ERR_STATE = 5,       /* call order violated (e.g. maxflow before build)           */
    MGC_ERR_UNSUPPORTED = 6, /* valid request outside the implemented path                */
    MGC_ERR_NOT_CONVERGED = 7
} mgc_status;

/* boundary terms, reference energy_voxel.py:68-516 */
typedef enum mgc_term {
    MGC_TERM_NONE = 0,
    MGC_TERM_DIFFERENCE_LINEAR = 1,      /* energy_voxel.py:117-191 */
    MGC_TERM_DIFFERENCE_EXPONENTIAL = 2, /* energy_voxel.py:241-302 */
    MGC_TERM_DIFFERENCE_DIVISION = 3,    /* energy_voxel.py:350-409 */
    MGC_TERM_DIFFERENCE_POWER = 4,       /* energy_voxel.py:455-516 */
    MGC_TERM_MAXIMUM_LINEAR = 5,         /* energy_voxel.py:68-114  */
    MGC_TERM_MAXIMUM_EXPONENTIAL = 6,    /* energy_voxel.py:194-238 */
    MGC_TERM_MAXIMUM_DIVISION = 7,       /* energy_voxel.py:305-347 (uses the difference skeleton, :347) */
    MGC_TERM_MAXIMUM_POWER = 8           /* energy_voxel.py:412-452 */
} mgc_term;

typedef enum mgc_dtype {
    MGC_U8 = 0, MGC_I8 = 1, MGC_U16 = 2, MGC_I16 = 3, MGC_U32 = 4, MGC_I32 = 5,
    MGC_U64 = 6, MGC_I64 = 7, MGC_F32 = 8, MGC_F64 = 9
} mgc_dtype;

/* termtype of the reference, lib/maxflow/src/graph.h:57-61 */
enum { MGC_SOURCE = 0, MGC_SINK = 1 };

typedef struct mgc_stats {
    double  build_ms;          /* device time of the last mgc_build                        */
    double  solve_ms;          /* device time of the last mgc_maxflow                      */
    double  discharge_ms;      /* ... of which tile-discharge kernels (HIP events)         */
    double  relabel_ms;        /* ... of which global-relabel kernels                      */
    int64_t discharge_launches;
    int64_t relabel_launches;
    int64_t discharge_tiles;   /* tile discharges executed                                 */
    int64_t relabel_tiles;     /* tile relabels executed                                   */
    int64_t global_relabels;
    int64_t phases;
    int64_t ntiles;
    int64_t nvox;
    int64_t device_bytes;      /* HBM held by the handle                                   */
    int64_t reserved[3];       /* [0]: counter read-backs (host syncs) of the solve; [1]: cycles of colour phases that ran on radial labels; [2]: tiles a surface of weak arcs passes through, as built */
    /* the dominant kernel by itself: discharge_ms / _launches / _tiles pool the one-wave-per-tile kernel (k_discharge_w) and the
     * workgroup-per-tile kernel that takes the short lists; these three are k_discharge_w alone */
    double  discharge_wave_ms;
    int64_t discharge_wave_launches;
    int64_t discharge_wave_tiles;
    int64_t timing_stride;     /* every n-th solver launch of a kind carries a HIP event pair; the _ms are their mean x launches */
    int64_t held_wakeups;      /* tile faces across which k_discharge_w left flow in the outbox without waking the neighbour (thin flow held back during
                                  the early cycles of a solve that floods against walls; 0 where the rule did not engage) */
    double  update_ms;         /* device time of the last t-link update (mgc_update_*): k_update_tlinks + its flow-constant sum; 0 after mgc_build.
                                  After mgc_edit_markers: plus its scatter kernel */
    double  delta_ms;          /* device time of the last mgc_labels_delta: compare + count + scan (+ the ordered write when the ids were delivered) */
} mgc_stats;

/* Invariants of a maximum preflow, checked on the device (mgc_validate).  The reference has the same idea as a debugging
 * aid: Graph::test_consistency, lib/maxflow/src/maxflow.cpp:610-682.  It is the only check available for volumes no CPU
 * oracle can reach (BASELINE.json configs 4 and 5).  Counts are over the OWNED voxels of the handle (a slab: its planes);
 * everything must be zero, the two errors of the order of rounding, and the two flow values equal -- summed over the
 * ranks first when the volume is cut into slabs. */
typedef struct mgc_validation {
    int64_t voxels;                 /* owned voxels looked at                                                     */
    int64_t negative_values;        /* a residual, an excess or a sink link below zero                            */
    int64_t active_excess;          /* excess on a voxel that can still reach the sink: the preflow is not maximum */
    int64_t residual_arcs_across;   /* residual arc from a voxel that cannot reach the sink to one that can       */
    int64_t sink_links_across;      /* residual sink link on a voxel labelled "cannot reach the sink"             */
    int64_t pair_violations;        /* rcap(u,v) + rcap(v,u) != cap(u,v) + cap(v,u) beyond rounding               */
    int64_t node_violations;        /* from the source != excess + into the sink + net outflow beyond rounding    */
    int64_t pending_outbox;         /* flow pushed across a tile face and not yet absorbed (6-neighbourhood)      */
    int64_t reserved[4];
    double  max_pair_error;         /* largest relative error of the two conservation checks                      */
    double  max_node_error;
    double  flow_into_sink;         /* sum over the owned voxels of (sink link as built - residual sink link)     */
    double  cut_capacity;           /* capacity of the cut the labels define, this handle's part (without the constant) */
    double  flow_constant;          /* the part add_tweights folds into the flow (graph.h:416-425), this handle's  */
    double  sink_capacity_used;     /* sum of the built sink links that carry flow.  flow_into_sink is a sum of differences
                                       (65535 - residual) and only known to about 1e-13 of this; cut_capacity is exact */
    double  reserved_d[2];
} mgc_validation;

/* number of usable devices (0 => every other call fails with MGC_ERR_NO_DEVICE) */
int mgc_device_count(int* count);
/* free / total HBM of a device in bytes (hipMemGetInfo): callers that size work by memory -- tests that need tens of GB skip instead
 * of failing on a smaller device; no reference counterpart (the reference malloc()s and exit(1)s, graph.cpp:19-23) */
int mgc_device_memory(int device, int64_t* free_bytes, int64_t* total_bytes);

/* Replaces GCGraph.__init__ -> GraphDouble(nodes, edges) + add_node (graph.py:294-308,
 * graph.cpp:12-31).  ndim 1..3; connectivity = 2*ndim (the only neighbourhood the reference supports,
 * generate.py:44-49) or 3^ndim - 1 (full neighbourhood: 8 in 2-D, 26 in 3-D -- an extension named by
 * BASELINE.json configs 3 and 5, weights = the same g(.) on every offset, spacing = Euclidean offset length). */
int mgc_create(int ndim, const int64_t* shape, int connectivity, int device, mgc_handle* out);
int mgc_destroy(mgc_handle h);
const char* mgc_last_error(mgc_handle h); /* h may be NULL: error of the last failed mgc_create */
/* Device memory of destroyed handles is kept in a per-device pool (blocks >= 1 MiB, by exact size, up to MEDPY_HIP_POOL_MB --
 * default an eighth of the device's memory; 0 switches the pool off) and handed to the next handle that asks for the same sizes:
 * the reference allocates per graph (graph.cpp:12-31, one graph per volume in bin/medpy_graphcut_voxel.py:163-182), and a 13 GB
 * handle per 512^3 volume is 0.5 - 0.8 s of hipMalloc / hipFree on some boxes.  An allocation that fails empties the pool first.
 * mgc_pool_trim returns everything to the driver; mgc_pool_info reports what is idle and how often the pool served a request. */
int mgc_pool_trim(int device);
int mgc_pool_info(int device, int64_t* idle_bytes, int64_t* hits, int64_t* misses);

/* Replaces boundary_<term>(graph, (image, sigma, spacing)) -> __skeleton_base
 * (energy_voxel.py:611-664).  `image` has the handle's shape.  p0: sigma for
 * exponential/division/power (for exponential pass sigma; the library squares it the way
 * math.pow does), unused for linear (the intensity range is reduced on the device).
 * spacing: ndim doubles or NULL (False). */
int mgc_set_boundary(mgc_handle h, int term, const void* image, int dtype, double sigma, const double* spacing);

/* Integer-valued images (CT, MR: uint8 / uint16 / int16, or floats that hold integers): the exponential and power terms
 * depend on the two intensities only through d = |I_p - I_q| (difference terms) or max(|I_p|, |I_q|) (maximum terms), an
 * integer below `n`.  table[d] = the boundary function of d as the REFERENCE evaluates it on the host -- NumPy's exp / pow,
 * energy_voxel.py:226-236, 290-300, 444-452, 506-513, floored at sys.float_info.min -- replaces the device's own exp / pow
 * (OCML, <= 2 ulp away): the n-link weights are then BIT-IDENTICAL to the reference's on such images.  The spacing division
 * still happens on the device (IEEE division).  Call after mgc_set_boundary (which forgets a table set earlier); n = 0
 * forgets it; n <= 65536; an intensity pair beyond the table falls back to the device's own evaluation. */
int mgc_set_boundary_lut(mgc_handle h, const double* table, int64_t n);

/* Replaces regional_probability_map(graph, (probability_map, alpha)) (energy_voxel.py:33-65)
 * -> set_tweights_all (graph.py:551-552).  dtype MGC_F32 or MGC_F64: products are evaluated in
 * that dtype, as NumPy does for the reference. */
int mgc_set_regional_probability(mgc_handle h, const void* probability_map, int dtype, double alpha);

/* Replaces set_source_nodes / set_sink_nodes over marker masks (generate.py:169-172,
 * graph.py:310-380): nonzero fg -> add_tweights(i, 65535, 0), nonzero bg -> add_tweights(i, 0, 65535). */
int mgc_set_markers(mgc_handle h, const uint8_t* fg, const uint8_t* bg);

/* WARM UPDATES of a built handle (the interactive loop: a stroke is added, the graph is cut again).  They replace the markers /
 * the regional term as mgc_set_markers / mgc_set_regional_probability do, but keep the residual graph in HBM: the n-links are
 * not touched, the new t-links are folded into the residual state, and the next mgc_maxflow continues from it.  Its
 * labels, flow and mgc_validate are those of mgc_build + mgc_maxflow of the same inputs (explicit merged t-links and plug-in
 * edges of the build included, unchanged).  Valid on a built handle before or after mgc_maxflow; MGC_ERR_STATE before
 * mgc_build, after a solve that returned MGC_ERR_NOT_CONVERGED, and on a slab handle.  mgc_set_markers /
 * mgc_set_regional_probability + mgc_build remain the cold rebuild. */
int mgc_update_markers(mgc_handle h, const uint8_t* fg, const uint8_t* bg);
int mgc_update_regional_probability(mgc_handle h, const void* probability_map, int dtype, double alpha);

/* EDITS BY LIST: the two ends of the interactive loop at the cost of the edit, not of the volume.
 *
 * mgc_edit_markers replaces set_source_nodes / set_sink_nodes called with node ids (generate.py:169-172) on a graph that is
 * already built: ids[k] = C-order flat voxel id, ops[k] = what happens to its markers: 1 = set the foreground marker, 2 = set the
 * background marker, 4 = clear the foreground marker, 8 = clear the background marker, or a sum of these (a voxel may carry both
 * markers, as with masks).  The mask planes resident in HBM are edited there by a scatter kernel -- 9 n bytes go up, a handle
 * built without one kind of marker gets a zeroed plane of that kind first -- and the new t-links are folded into the residual
 * state exactly as by mgc_update_markers: the handle is afterwards in the state mgc_update_markers with the equivalent full masks
 * leaves it in, and a later mgc_build (cold rebuild) sees the edited masks.  States as for mgc_update_markers (MGC_ERR_STATE
 * before mgc_build, after a solve that did not converge, on a slab handle).  MGC_ERR_INVALID, with mgc_last_error naming the first
 * offending entry, for an id outside [0, nvox), ops == 0, ops > 15, set and clear of the same marker in one entry (1|4, 2|8) and
 * for an id that is in the list twice; a refused call leaves the handle exactly as it was.  The list is checked on the host before
 * anything is written (a list that does not ascend strictly is sorted in a copy to find repeated ids): an edit of more than a
 * fraction of the volume is better sent as masks.  n == 0 is MGC_OK and changes nothing, a finished solve included.
 *   If the handle holds a finished solve when the edit arrives, the label volume of that solve is first put aside in HBM (one
 * byte per voxel, allocated on the first such call and kept with the handle; MGC_ERR_OOM before anything changed if it cannot be
 * had).  Further edits before the next solve keep that copy.  mgc_build, mgc_update_markers and mgc_update_regional_probability
 * drop it.
 *
 * mgc_get_markers: the resident masks, 0 / 1 per voxel; either pointer may be NULL, a kind the handle does not hold reads as
 * zeros.  How a caller who only ever sent lists saves a session.
 *
 * mgc_labels_delta replaces the what_segment loop over all voxels (bin/medpy_graphcut_voxel.py:177-181) after an edit: after
 * mgc_maxflow on a handle that holds the labels of the solve before the edit(s), *n = the number of voxels whose label differs
 * from that solve's, and if *n <= cap, ids[0 .. *n) = their flat ids in ascending order (a label is one bit: new = old ^ 1).  If
 * *n > cap nothing is written to ids and the call still returns MGC_OK: size a buffer and ask again, or fall back to mgc_labels.
 * The two label volumes are compared on the device; 8 *n bytes and the count come down.  Changes no state, may be repeated.
 * MGC_ERR_STATE when the handle is not solved or holds no such labels. */
int mgc_edit_markers(mgc_handle h, int64_t n, const int64_t* ids, const uint8_t* ops);
int mgc_get_markers(mgc_handle h, uint8_t* fg, uint8_t* bg);
int mgc_labels_delta(mgc_handle h, int64_t cap, int64_t* ids, int64_t* n);

/* WARM UPDATE OF THE BOUNDARY TERM: the n-link side of the interactive loop (a cut leaks, sigma comes down, the graph is cut
 * again; DESIGN 10, "The boundary term").  Arguments as for mgc_set_boundary; image == NULL keeps the resident image and its
 * dtype (another sigma, term or spacing: nothing is uploaded), otherwise the new image goes up next to the old one, which is
 * released after the update.  The capacities as built are a pure function of the resident image, so one kernel evaluates every
 * arc's capacity under the old and under the new arguments and folds the change into the residual graph: flow that no longer
 * fits an arc goes back to its tail as excess and is taken from its head as residual sink capacity.  The next mgc_maxflow is a
 * warm solve; its labels, flow and mgc_validate are those of mgc_set_boundary + mgc_build + mgc_maxflow of the new arguments.  The
 * *_linear terms measure the range of a new image again.
 *   mgc_update_boundary_lut hands over the table of the NEW arguments (mgc_set_boundary_lut) and is called BEFORE the
 * mgc_update_boundary it belongs to, which consumes it: the table the graph was built with stays readable until the update has
 * run.  Without it the new term is evaluated without a table.  MGC_ERR_STATE from mgc_update_boundary if the new term has none.
 *   States as for mgc_update_markers (MGC_ERR_STATE before mgc_build, after a solve that did not converge, on a slab handle);
 * MGC_ERR_UNSUPPORTED on a handle whose capacities the image does not determine (explicit edges, dense weight arrays), on a
 * handle built without a boundary term, and for term == MGC_TERM_NONE.  A handle whose n-links were edited by arc list
 * (mgc_edit_nweights) holds its capacities as built from the first such edit on and is refused for the same reason, until
 * the end of its life.  A refused call leaves the handle as it was.  If the
 * handle holds a finished solve its labels are put aside as by mgc_edit_markers: mgc_labels_delta after the next mgc_maxflow
 * reports what the new arguments flipped.
 *   mgc_get_boundary_update_info: of the last update, out4 = {arcs whose capacity changed, arcs whose flow no longer fitted,
 * voxels whose excess or residual sink link changed, tiles that gained a t-link flag}. */
int mgc_update_boundary(mgc_handle h, int term, const void* image, int dtype, double sigma, const double* spacing);
int mgc_update_boundary_lut(mgc_handle h, const double* table, int64_t n);
int mgc_get_boundary_update_info(mgc_handle h, int64_t* out4);

/* EDITS OF N-LINKS BY ARC LIST: the local n-link correction of the interactive loop -- a barrier drawn where the cut leaked
 * through a gap in the edge map, glue across a spurious edge ("Edits of n-links by list").  Arguments as for
 * mgc_add_edges, but with REPLACE semantics: after the call the capacity as built of the arc i[k] -> j[k] is cap[k] and that of
 * j[k] -> i[k] is rev[k] (rev == NULL: rev = cap).  0 makes a one-way arc or, both ways, a barrier.  Only the listed arcs are
 * touched: the flow the residual graph holds on them is clamped to the new capacities, what no longer fits goes back to the
 * arcs' ends as signed excess (Kohli & Torr's dynamic graph cuts, directed form), and the next mgc_maxflow is a warm solve with
 * the labels, flow and mgc_validate of a cold build of the edited capacities.  Valid on a built handle before or after
 * mgc_maxflow, both neighbourhoods, whatever the capacities came from (built-in term, dense arrays, explicit edges).
 *   States as for mgc_update_markers: MGC_ERR_STATE before mgc_build, on a slab handle, after a solve that did not converge.
 * n == 0 is MGC_OK and changes nothing, a finished solve included.  The list is checked on the host before anything is
 * written, and a refused call leaves the handle exactly as it was: MGC_ERR_INVALID for an id outside [0, nvox), a capacity
 * that is not finite and >= 0, and an unordered pair that is in the list twice (in either orientation); MGC_ERR_UNSUPPORTED
 * for (i, j) that are not neighbours of the handle's lattice; mgc_last_error names the first offending entry.
 *   A handle whose capacities the image determines gets them written out on the first edit (8 * ndir bytes per voxel, as for
 * explicit edges; MGC_ERR_OOM before anything changed if that cannot be had), and stays such a handle: mgc_update_boundary
 * refuses it from then on.
 *   The edits stay with the handle as a list on the host, keyed by the pair; a later edit of a pair replaces the earlier one.
 * mgc_build applies the list last -- boundary term, dense store, batch of mgc_add_edges, then these (replace) -- so a cold rebuild
 * after new markers or another sigma keeps the barriers.  mgc_clear_nweight_edits forgets the list and makes the handle unbuilt,
 * as mgc_clear_nweights does.
 *   If the handle holds a finished solve its labels are put aside as by mgc_edit_markers: mgc_labels_delta after the next
 * mgc_maxflow reports what the edit flipped; further edits before that solve keep the copy.  After a call that went through,
 * mgc_last_error holds a note of where its device time went (cap0_fill_ms, fold_ms, refresh_ms).
 *   mgc_get_nweight_edit_info: out4 = {pairs in the list, and of the last mgc_edit_nweights: pairs whose capacity changed
 * bitwise, arcs whose flow no longer fitted, voxels whose excess or residual sink link changed}. */
int mgc_edit_nweights(mgc_handle h, int64_t n, const int64_t* i, const int64_t* j, const double* cap, const double* rev);
int mgc_clear_nweight_edits(mgc_handle h);
int mgc_get_nweight_edit_info(mgc_handle h, int64_t* out4);

/* After mgc_maxflow (or the slab driver's last step): see mgc_validation.  Also works on a graph whose solve was cut
 * short (MGC_ERR_NOT_CONVERGED): it then reports the excess that is still active.  MGC_ERR_STATE before the first solve
 * step of a build: the distance labels it reads do not exist yet. */
int mgc_validate(mgc_handle h, mgc_validation* out);

/* The *_linear terms divide by the intensity range of the image (energy_voxel.py:101: max |I|; 174-176:
 * |max - min| in the image's dtype).  A single handle measures it itself.  A SLAB only holds its own planes, so the
 * caller reduces the local triples {min, max, max|.|} over the ranks (min, max, max) and hands the global one back
 * before mgc_build; building a *_linear slab without it fails with MGC_ERR_STATE.  NULL forgets a range set earlier;
 * mgc_set_boundary does so too.  max|.| is numpy.abs(image).max() in the image's own dtype: the minimum of a signed
 * integer type wraps onto itself there and counts with its negative value. */
int mgc_get_image_range(mgc_handle h, double* out3);
int mgc_set_image_range(mgc_handle h, const double* in3);

/* Plug-in path (user supplied energy callables drive GCGraph.set_nweight / set_tweight,
 * graph.py:382-440, 466-498).  Edges must join lattice neighbours (checked here: MGC_ERR_UNSUPPORTED
 * names the first edge that does not; arbitrary graphs go to msg_*); capacities accumulate like
 * sum_edge (graph.h:457-480): an edge given several times adds up IN CALL ORDER on top of the boundary
 * term's weight, the same floating point additions as the reference.  One batch per build (a later
 * batch replaces one that a build already applied); the batch stays with the handle, so a rebuild
 * applies it again.  t-weights: tr[n] = merged residual per node, flow_const = the
 * part add_tweights folds into the flow (graph.h:416-425); applied before the markers. */
int mgc_add_edges(mgc_handle h, int64_t n, const int64_t* i, const int64_t* j, const double* cap, const double* rev);
int mgc_set_tweights_merged(mgc_handle h, const double* tr, double flow_const);

/* Dense n-link weight arrays: the bulk form of the plug-in path, for boundary terms the caller evaluates itself (a gradient
 * map, a learned edge probability, a directed penalty).  `offset` has ndim components in {-1,0,1} and must be a neighbour of
 * the handle's lattice (rule and error of mgc_get_nweights_offset); `there` and `back` are C-contiguous arrays of the handle's
 * shape, dtype MGC_F32 or MGC_F64 (f32 is widened on the device), in the layout mgc_get_nweights_offset returns: there[p] is
 * added to the capacity of the arc p -> p + offset, back[p] to the capacity of the arc p + offset -> p.  Entries whose
 * p + offset lies outside the volume are ignored whatever they hold.  back == NULL: `there` is used both ways.
 *   Semantics of sum_edge (graph.h:457-480): calls accumulate per arc in call order with sequential f64 adds, so with no
 * built-in term and one call per offset the capacity is 0.0 + w == w bit for bit.  A build applies, in this order: the
 * boundary term's weight, then these arrays, then the batch of mgc_add_edges.  The arrays are kept on the device in a
 * tile-major store that stays with the handle (8 * ndir bytes per voxel, allocated by the first call; a direction that is
 * given again costs 8 bytes per voxel more, so that the adds keep their order), and the capacities as built are materialised
 * as for explicit edges (another 8 * ndir bytes per voxel): a rebuild applies the store again, mgc_clear_nweights forgets and
 * frees it.  Either call on a built handle makes it unbuilt, as mgc_add_edges does.
 *   Every entry that is not ignored must be finite and >= 0 (zero: a one-way arc).  The arrays are checked on the device before
 * the store is written: MGC_ERR_INVALID, with mgc_last_error naming the flat index and the value of the first offender, and the
 * handle exactly as it was.  MGC_ERR_UNSUPPORTED on a slab handle.  After a call that went through, mgc_last_error holds a note
 * of where its time went (upload_ms, check_ms, accumulate_ms).
 *   A 6-connected graph with such arrays, no batch of explicit edges, and every arc inside the volume residual after the build
 * starts its first solve with the distance transform, like a graph of a built-in term. */
int mgc_add_nweights(mgc_handle h, const int* offset, const void* there, const void* back, int dtype);
int mgc_clear_nweights(mgc_handle h);

/* Dense t-link weight arrays: the bulk form of GCGraph.set_tweight (graph.py:466-498), for regional terms the caller evaluates
 * itself (negative log-likelihoods of a mixture model or a histogram, the output of a network); DESIGN 12.  `source` and `sink`
 * are C-contiguous arrays of the handle's shape, dtype MGC_F32 or MGC_F64 (f32 is widened on the device, which is exact).
 *   Semantics of Graph::add_tweights (graph.h:416-425), one call per voxel on the handle's explicit t-link: calls accumulate in
 * call order, the part both weights share goes into the flow constant.  Negative weights are allowed, as in the reference; every
 * entry must be finite.  The arrays are checked on the device before the first write: MGC_ERR_INVALID, with mgc_last_error
 * naming the array, the flat index and the value of the first offender, and the handle exactly as it was.
 *   The first call allocates the STORE that stays with the handle: two f64 per voxel in C order -- the merged explicit t-link,
 * which builds and warm updates read where they read the vector of mgc_set_tweights_merged, and the voxel's share of the flow
 * constant -- plus one partial sum per 4096 voxels.  The flow constant of the store is the sum of the share plane in a fixed
 * order.  The merge order of a build stays: explicit t-links, regional probability map, fg markers, bg markers.  The call makes
 * a built handle unbuilt.  mgc_clear_tweights forgets and frees the explicit t-links (of either origin) and makes the handle
 * unbuilt.  MGC_ERR_UNSUPPORTED on a slab handle.  After a call that went through, mgc_last_error holds a note of where its
 * time went (upload_ms, check_ms, accumulate_ms).
 *   The store and mgc_set_tweights_merged are exclusive on one handle (a merged vector comes with a flow constant whose
 * per-voxel shares are unknown): whichever comes second returns MGC_ERR_STATE until mgc_clear_tweights.
 *   mgc_update_tweights: the warm form, on a built handle (states as for mgc_update_markers).  Afterwards the store holds
 * exactly what mgc_clear_tweights and one mgc_add_tweights of these arrays leave, the change of every voxel's merged t-link is
 * folded into the residual graph as by mgc_update_markers, and the next mgc_maxflow is a warm solve.  Checked before the first
 * write.  Drops the label snapshot of mgc_labels_delta.
 *   mgc_edit_tweights: by voxel list, REPLACE as mgc_edit_nweights: afterwards the explicit t-link of voxel ids[k] is what one
 * add_tweights of (source[k], sink[k]) leaves on a zero t-link: tr = source - sink, share min(source, sink).  A handle without a
 * store gets a zeroed one first (MGC_ERR_OOM before anything changed).  The list is checked on the host before the first write:
 * MGC_ERR_INVALID for an id outside [0, nvox), a weight that is not finite, an id given twice; mgc_last_error names the first
 * offending entry.  n == 0 is MGC_OK and changes nothing, a finished solve included.  MGC_ERR_STATE before mgc_build, on a slab
 * handle, after a solve that did not converge, and when the explicit t-links came from mgc_set_tweights_merged.  The labels of
 * a finished solve are put aside as by mgc_edit_markers, so mgc_labels_delta works after the next solve.  The edits live in the
 * store: a later mgc_build sees them.
 *   mgc_get_tweight_edit_info: out4 = {store held (0 / 1), dense calls accumulated since the last clear, entries of the last
 * list call, voxels whose explicit t-link changed bitwise in the last update or edit}. */
int mgc_add_tweights(mgc_handle h, const void* source, const void* sink, int dtype);
int mgc_clear_tweights(mgc_handle h);
int mgc_update_tweights(mgc_handle h, const void* source, const void* sink, int dtype);
int mgc_edit_tweights(mgc_handle h, int64_t n, const int64_t* ids, const double* source, const double* sink);
int mgc_get_tweight_edit_info(mgc_handle h, int64_t* out4);

/* The binned regional term: t-links that depend on a voxel only through the BIN of its intensity -- the negative log-likelihoods
 * of the intensity histograms under the markers (Boykov & Jolly), of a mixture model evaluated per bin, any table; DESIGN 14.
 * What a stroke changes of such a term is two tables of a few hundred entries, so the term is fitted and expanded on the device:
 * no per-voxel array crosses the bus.
 *   The rule (medpy_amd/csrc/mgc_binned.h): bin(v) = clamp(floor((double(v) - lo) / width), 0, nbins - 1), one f64 subtraction,
 * one IEEE f64 division and a floor, bit for bit numpy.clip(numpy.floor((image.astype(float64) - lo) / width), 0, nbins - 1).
 * 1 <= nbins <= 65536, lo finite, width finite and > 0.
 *   mgc_set_feature_image: the scalar image the bins are taken of, a C-contiguous array of the handle's shape in any image dtype
 * (MGC_U8 .. MGC_F64), uploaded and kept with the handle (counted in device_bytes); NULL forgets it and gives the bytes back.
 * Where none is set the calls below read the image of mgc_set_boundary (the maximum_* terms take a gradient image: then a feature
 * image is needed).  No effect on mgc_build or on any other call; a built handle stays built.
 *   mgc_marker_histograms: fg_hist[b] / bg_hist[b] (nbins entries each) = the voxels of bin b under the fg plane / under the bg
 * plane the handle holds now (mgc_set_markers, mgc_update_markers, mgc_edit_markers); a voxel under both counts in both, a
 * plane that was never given counts nothing.  out4 (or NULL) = {counts under fg, counts under bg, counts the clamp raised into
 * bin 0 (value below lo), counts the clamp lowered into the last bin (value at or above lo + nbins * width)}.  Exact integers,
 * whatever the order of the adds.  Valid before and after mgc_build; changes nothing on the handle.
 *   mgc_add_tweights_binned: leaves the store exactly as mgc_add_tweights(h, S, K, MGC_F64) would with S[p] = source_table[bin(p)]
 * and K[p] = sink_table[bin(p)] -- the same add_tweights on top of what the store holds, the same share plane, the same
 * fixed-order flow constant, the same count of dense calls, the same states, and a note of where its time went (check_ms,
 * expand_ms, flow_const_ms) in mgc_last_error.  mgc_update_tweights_binned: the warm form, exactly mgc_update_tweights of the
 * expanded arrays (the store replaced, the changed voxels counted, the change folded into the residual graph, the label
 * snapshot dropped; its states); its note adds fold_ms.
 *   Refusals, all before anything is written, the handle exactly as it was: MGC_ERR_INVALID for nbins, lo or width out of range,
 * a NULL table, a table entry that is not finite (negative entries are allowed; mgc_last_error names table and index) and a value
 * of a float image that is not finite (flat index and value; mgc_marker_histograms looks only under the markers);
 * MGC_ERR_STATE without a feature image and without a boundary image, and in the states of mgc_add_tweights /
 * mgc_update_tweights; MGC_ERR_UNSUPPORTED on a slab handle; MGC_ERR_OOM before anything changed. */
int mgc_set_feature_image(mgc_handle h, const void* image, int dtype);
int mgc_marker_histograms(mgc_handle h, int64_t nbins, double lo, double width, int64_t* fg_hist, int64_t* bg_hist, int64_t* out4);
int mgc_add_tweights_binned(mgc_handle h, int64_t nbins, double lo, double width, const double* source_table, const double* sink_table);
int mgc_update_tweights_binned(mgc_handle h, int64_t nbins, double lo, double width, const double* source_table, const double* sink_table);

/* The histograms of EVERY voxel, split by a label: what fitting the binned term to a segmentation instead of the strokes needs (the
 * iterated graph cut of GrabCut).  fg_hist[b] / bg_hist[b] (nbins entries each) = the voxels of bin b whose label is not
 * zero / is zero; the image and the rule of the bin are those of mgc_marker_histograms.  out4 (or NULL) = {voxels with a label,
 * voxels without, counts the clamp raised into bin 0, counts the clamp lowered into the last bin}.  Exact integers, whatever the
 * order of the adds: numpy.bincount of the bins under the labels and under their complement.
 *   labels NULL: the labels of the handle's current cut, read where they lie on the device -- valid in the states of mgc_cut_sets
 * (built, solved to a maximum preflow, no update or edit waiting for the next mgc_maxflow), MGC_ERR_STATE otherwise.  labels given:
 * one byte per voxel in C order on the host, not zero = foreground; the plane goes up into a block that is given back before the
 * call returns, and the call is valid wherever the handle holds an image, before mgc_build too.
 *   Refusals, all before anything is written: MGC_ERR_INVALID for nbins, lo or width out of range, for fg_hist or bg_hist NULL and
 * for a value of a float image that is not finite ANYWHERE in the volume (the lowest flat index and the value are named: every
 * voxel is counted here); MGC_ERR_STATE without a feature image and without a boundary image; MGC_ERR_UNSUPPORTED on a slab
 * handle.  Changes nothing on the handle: labels, label snapshot, residual graph, statistics, launch counts and device_bytes stay. */
int mgc_label_histograms(mgc_handle h, const uint8_t* labels, int64_t nbins, double lo, double width, int64_t* fg_hist, int64_t* bg_hist, int64_t* out4);

/* The connected components of a label plane on the handle's lattice, found on the device.  The plane is the labels of
 * the current cut (labels NULL; the states of mgc_cut_sets) or one byte per voxel in C order on the host, any byte but 0 being
 * foreground (any single handle, built or not).  side 1 takes the components of the foreground, 0 those of the background; full 0
 * the face neighbourhood (2 / 4 / 6 neighbours), 1 the full one (2 / 8 / 26).  Neighbours outside the volume do not exist.
 *   The components are numbered 1 .. K by their FIRST voxel, the smallest voxel id they hold: the numbering of
 * scipy.ndimage.label.  ids (nvox entries or NULL): the number of every voxel's component, 0 on the other side.  first / size /
 * flags (cap entries each; NULL allowed when cap is 0): row k - 1 describes component k -- first voxel, voxel count, and flag bits
 * 1 = holds a foreground marker of the handle, 2 = holds a background marker, 4 = touches the border of the volume (some coordinate
 * 0 or dim - 1 among the axes of extent > 1).  When K > cap the table holds the first cap components and the call still succeeds:
 * look at K and call again.
 *   out8 (or NULL) = {K, voxels of side, size of the largest component, its id (ties: the smaller id), tiles decided by their
 * label summary, tiles processed, cross-tile unions attempted, longest parent walk seen}.
 *   Refusals, all before anything is written: MGC_ERR_INVALID for a NULL handle, a side or full other than 0 / 1, a negative cap
 * or a table pointer missing with cap > 0; MGC_ERR_UNSUPPORTED on a slab handle and for volumes of 2^32 - 1 voxels or more (parents
 * are 32-bit); MGC_ERR_STATE with labels NULL outside the states of mgc_cut_sets.  Changes nothing on the handle: every block of the
 * call comes from the pool and goes back; labels, snapshot, markers, residual graph, statistics, launch counts, device_bytes stay. */
int mgc_components(mgc_handle h, const uint8_t* labels, int side, int full, int32_t* ids, int64_t cap, int64_t* first, int64_t* size, uint8_t* flags, int64_t* out8);

/* A label plane cleaned by components, in two steps.  1: of the foreground components at the fg_full neighbourhood those
 * PASS that hold at least min_size (>= 1) voxels and, if seeded, a foreground marker of the handle; if largest > 0 only the `largest`
 * biggest of them survive, ties on size going to the smaller id (0: no limit).  2, if fill_holes: the background components of the
 * result at the hole_full neighbourhood that neither touch the border of the volume nor hold a background marker become foreground.
 *   out (nvox bytes or NULL): the cleaned plane, 0 / 1.  changed_ids (cap entries or NULL): the ascending ids of the voxels whose
 * being foreground changed.  out8 (or NULL) = {foreground components, survivors, voxels removed, cavities filled, voxels filled,
 * voxels changed, 1 if the list was written (0: more than cap, or no list asked for: only the count is valid), 0}.
 *   The plane, the states and the side effects (none) are those of mgc_components; MGC_ERR_INVALID also for a NULL rule,
 * min_size < 1, largest < 0, a rule flag other than 0 / 1, a negative cap. */
typedef struct { int32_t fg_full, seeded, fill_holes, hole_full; int64_t min_size, largest; } mgc_clean_rule;
int mgc_clean_labels(mgc_handle h, const uint8_t* labels, const mgc_clean_rule* rule, uint8_t* out, int64_t cap, int64_t* changed_ids, int64_t* out8);

/* The exact Euclidean distance transform of a byte plane on the handle's lattice, and the overlap and surface measures of two planes
 * (DESIGN 17): what scoring a cut against a ground truth needs, where the cut lies.  A plane is one byte per voxel in C order on the
 * host, any byte but 0 being foreground (any single handle, built or not), or NULL: the labels of the current cut (the states of
 * mgc_cut_sets, MGC_ERR_STATE otherwise).  spacing: NULL = unity, else ndim finite positive doubles, one per axis of the handle.
 *   mgc_distance_transform: the seeds are the voxels of `side` (1: not zero, 0: zero).  out_sq[v] (nvox doubles in C order, or NULL:
 * only the counts) = the minimum over the seeds s of fl(fl(fl(a_{n-1}^2) + fl(a_{n-2}^2)) + fl(a_{n-3}^2)), a_k = fl(spacing_k *
 * (v_k - s_k)): the SQUARED distance in f64, the axes added from the last to the first, every operation rounded on its own (no fused
 * multiply-add).  0 on the seeds, +inf everywhere without a seed.  out4 (or NULL) = {seeds, lines that were longer than the 512
 * voxels a panel of on-chip memory takes and went the slower way through device memory, 0, 0}.
 *   mgc_surface_distances: the border of an object X at `connectivity` (1 .. ndim, the structuring element of
 * scipy.ndimage.generate_binary_structure(ndim, connectivity)) is every voxel of X with a neighbour that is background or outside the
 * volume -- X ^ binary_erosion(X, structure).  Only the axes of the handle give neighbours: a 2-D handle has none along z, a 3-D handle
 * of shape (1, Y, X) has them, all outside.  sds_sq (cap doubles; NULL allowed when cap is 0) takes the SQUARED distance from each border
 * voxel of a to the nearest border voxel of b, in ascending voxel id, the first cap of them; the caller takes the root.  out8 (or NULL) =
 * {border voxels of a, border voxels of b, voxels of a, voxels of b, lines that went the slower way, 0, 0, 0}.  An empty a or b is no
 * error: nothing is written and the counts say so.  b must not be NULL.
 *   mgc_overlap_counts: out4 = {tp, fp, fn, tn} of a against b: voxels of both, of a only, of b only, of neither.  Exact integers,
 * summed in a fixed order.
 *   Refusals, all before anything is written: MGC_ERR_INVALID for a NULL handle, a side other than 0 / 1, a connectivity outside
 * 1 .. ndim, a spacing that is not finite and positive, a negative cap, sds_sq NULL with cap > 0, b or the out4 of mgc_overlap_counts
 * NULL; MGC_ERR_UNSUPPORTED on a slab handle; MGC_ERR_STATE with a NULL plane outside the states of mgc_cut_sets.  Changes nothing on
 * the handle: every block of a call comes from the pool and goes back; labels, snapshot, markers, residual graph, statistics, launch
 * counts, device_bytes stay. */
int mgc_distance_transform(mgc_handle h, const uint8_t* plane, int side, const double* spacing, double* out_sq, int64_t* out4);
int mgc_surface_distances(mgc_handle h, const uint8_t* a, const uint8_t* b, int connectivity, const double* spacing, int64_t cap, double* sds_sq, int64_t* out8);
int mgc_overlap_counts(mgc_handle h, const uint8_t* a, const uint8_t* b, int64_t* out4);

/* The geodesic distance transform on the lattice of a single handle, and the regional term on top of it (the definition is
 * medpy_amd/csrc/mgc_geo.h).  full = 0: the face neighbourhood (2 / 4 / 6 neighbours), 1: the full one (2 / 8 / 26); neighbours outside
 * the volume do not exist.  The arc between the neighbours p and q = p + d has the length, in f64 and every operation rounded on its
 * own, w = e_d + gamma * |I_p - I_q| with e_d = step * sqrt(a_x^2 + a_y^2 + a_z^2) (x, the last array axis, first) and a_k =
 * spacing_k * |d_k|; spacing NULL: unity, else ndim finite positive values; gamma and step finite and not negative; step = 0 gives the
 * pure intensity geodesic.  I is the image of mgc_marker_histograms as f64 (the feature image, else the boundary image; every dtype);
 * with gamma = 0 no image is read and none is needed.  D(v) = the minimum over the seeds and the lattice paths from a seed to v of the
 * sum of the arc lengths added from the seed outwards: 0 on seeds, +inf where no seed connects -- the numbers of Dijkstra's algorithm
 * with f64 additions, bit for bit, whatever the order in which the device relaxes (D is a least fixpoint).
 *   mgc_geodesic_distance: source 0: seeds is a byte plane of the caller's (host, C order, any byte but 0 a seed; any single handle
 * will do, built or not); source 1 / 2: the foreground / background markers where they lie on the device, seeds NULL (a plane that
 * was never given has no seeds).  out: nvox doubles in C order or NULL.  out8 (or NULL) = {seeds, rounds (launches over the active
 * tiles), tile visits, in-tile sweeps summed, visits that ended at the sweep cap, voxels with a finite distance, 0, 0}.  Changes
 * nothing on the handle: every block of a call comes from the pool and goes back; labels, snapshot, markers, residual graph,
 * statistics, launch counts, device_bytes stay.
 *   mgc_add_tweights_geodesic: with D_F and D_B the transforms of the handle's foreground and background markers and t = D_F + D_B,
 * voxel p gets one Graph::add_tweights(S, K): both infinite: (0, 0); only D_F infinite: (0, lam); only D_B infinite: (lam, 0); t == 0:
 * (lam / 2, lam / 2); else (lam * (D_B / t), lam * (D_F / t)); lam finite and not negative.  The store is left exactly as
 * mgc_add_tweights(h, S, K, MGC_F64) would leave it.  mgc_update_tweights_geodesic is the warm form: mgc_update_tweights of
 * those arrays, except that the label snapshot of mgc_labels_delta is kept the way mgc_edit_tweights keeps it (the labels of a finished
 * cut change hands; the snapshot of an edit the next solve has yet to see stays): a refit follows a stroke, and mgc_labels_delta after
 * the next solve names the voxels the round changed.  The two planes live for the call only.  After a call that went through, mgc_last_error holds a note of where its
 * time went (transform_ms, expand_ms, flow_const_ms, fold_ms; rounds and visits of the two transforms).
 *   Refusals, before the first write and with the handle as it was: MGC_ERR_INVALID for a NULL handle, source outside 0..2, seeds NULL
 * with source 0 or given with source 1 / 2, full other than 0 / 1, gamma, step or lam not finite or negative, a spacing not finite and
 * positive, a value of a float image that is not finite (the message names the lowest flat index and the value); MGC_ERR_STATE with
 * gamma > 0 and no image, and in the states in which mgc_add_tweights / mgc_update_tweights refuse; MGC_ERR_UNSUPPORTED on a slab
 * handle; MGC_ERR_OOM before anything changed. */
int mgc_geodesic_distance(mgc_handle h, const uint8_t* seeds, int source, int full, double gamma, double step, const double* spacing, double* out, int64_t* out8);
int mgc_add_tweights_geodesic(mgc_handle h, int full, double gamma, double step, const double* spacing, double lam);
int mgc_update_tweights_geodesic(mgc_handle h, int full, double gamma, double step, const double* spacing, double lam);

/* Anisotropic diffusion of an image (Perona-Malik, options 1 and 2; Tukey's biweight, option 3) on the device: MedPy's
 * medpy.filter.smoothing.anisotropic_diffusion (the definition is medpy_amd/csrc/mgc_diffuse.h, stated there once).  The
 * image is converted to float32, every operation of an iteration is an IEEE float32 operation rounded on its own, and one launch
 * advances the whole volume by one iteration between two float32 buffers.  Options 2 and 3 equal the reference value for value;
 * option 1 takes exp in f64 and rounds it once, which is close to NumPy's float32 exp and not equal.  kappa finite and > 0, gamma
 * finite, spacing NULL (unity) or ndim finite positive values, niter >= 0 (0: the float32 copy).
 *   mgc_diffuse_image: handle-free, like msg_region_sums: image is the caller's (host, C order, ndim 1..3, any dtype MGC_U8 ..
 * MGC_F64), out nvox floats; the blocks come from the device's pool and are all given back.
 *   mgc_diffuse: on a single handle; the image is the one mgc_marker_histograms reads (the feature image, else the boundary image),
 * where it lies on the device.  keep = 0: nothing on the handle changes (labels, residual graph, statistics, launch counts,
 * device_bytes stay; the pool gets every block back).  keep = 1: the result becomes the handle's feature image as MGC_F32, exactly
 * as if mgc_set_feature_image had uploaded it (counted in device_bytes, replacing an earlier one): the histogram and geodesic
 * terms then read the smoothed image without it crossing the bus; out may be NULL.
 *   out4 (or NULL) = {iterations run, bricks per launch, 0, 0}.  After a call that went through, mgc_last_error (of the handle;
 * of NULL for mgc_diffuse_image) holds a note of where its time went (upload_ms, iterate_ms, download_ms).
 *   Refusals, before anything is written: MGC_ERR_INVALID for ndim outside 1..3, an extent < 1, a NULL image or shape, a bad dtype,
 * niter < 0, option outside 1..3, kappa not finite or <= 0, gamma not finite, a spacing not finite and positive, keep other than
 * 0 / 1, out NULL with keep = 0; MGC_ERR_STATE for a handle without any image; MGC_ERR_UNSUPPORTED on a slab handle; MGC_ERR_OOM
 * before anything changed. */
int mgc_diffuse_image(int device, int ndim, const int64_t* shape, const void* image, int dtype, int niter, double kappa, double gamma, const double* spacing, int option,
                      float* out, int64_t* out4);
int mgc_diffuse(mgc_handle h, int niter, double kappa, double gamma, const double* spacing, int option, int keep, float* out, int64_t* out4);

/* The seeded watershed of an image on the device, and the minima its markers are made from: the two steps of MedPy's
 * medpy_watershed.py between an image and the region image that graph_from_labels takes (the definition is
 * medpy_amd/csrc/mgc_ws.h, stated there once).  Both are handle-free, like mgc_diffuse_image: image is the caller's (host, C order,
 * ndim 1..3, dtype MGC_U8 .. MGC_I32 or MGC_F32), the work runs on a stream of its own, every block comes from the device's pool and
 * all are given back.  Only image values are compared, nothing is rounded: the results are a definition, not an approximation.
 *   mgc_watershed_image: markers nvox int32 (0: none, > 0: a label), mask nvox bytes (0: outside) or NULL, labels_out nvox int32.
 * Face neighbourhood.  Every voxel gets the arrival key (H, D) -- H the level at which water from a marker reaches it (the lowest
 * highest value of a path), D the steps since the path last rose -- as the least fixpoint of a relaxation over tiles, takes the
 * neighbour with the smallest (key, index) below its own as parent, and the marker at the root of its chain as label; 0 outside
 * the mask and where no marker connects.  A marker outside the mask is no marker.  On images without ties this is Meyer's
 * priority flood; on plateaus the regions meet where the step counts meet.
 *   out8 (or NULL) = {seed voxels, rounds (launches of the tile kernel), tile visits, sweeps, visits that ended at the sweep cap,
 * reached voxels (the seeds among them), pointer-jumping rounds, 0}.
 *   mgc_local_minima_image: mask_out[p] = (image[p] == scipy.ndimage.minimum_filter(image, size=size)[p]) (border `reflect`, the
 * window placed as SciPy places it for even and odd sizes), nvox bytes; out4 (or NULL) = {minima, 0, 0, 0}.
 *   After a call that went through, mgc_last_error(NULL) holds a note of where its time went (upload_ms, flood_ms, parent_ms,
 * resolve_ms, download_ms; upload_ms, filter_ms, download_ms).
 *   Refusals, before the first allocation: MGC_ERR_INVALID for ndim outside 1..3, an extent < 1, a NULL image, shape, markers or
 * result, a bad dtype, a negative marker, size < 1, a float value that is not finite; MGC_ERR_UNSUPPORTED for the 64-bit dtypes
 * (rank the values on the host and send MGC_U32) and for volumes of 2^32 - 1 voxels or more; MGC_ERR_OOM before anything changed. */
int mgc_watershed_image(int device, int ndim, const int64_t* shape, const void* image, int dtype, const int32_t* markers, const uint8_t* mask, int32_t* labels_out, int64_t* out8);
int mgc_local_minima_image(int device, int ndim, const int64_t* shape, const void* image, int dtype, int size, uint8_t* mask_out, int64_t* out4);

/* Runs the n-link / t-link kernels: the residual graph is now resident in HBM. */
int mgc_build(mgc_handle h);

/* Energy read-back for parity tests: axis weights in the layout of
 * `neighbourhood_intensity_term` (energy_voxel.py:644-658); tr_cap per node (Graph::get_trcap). */
int mgc_get_nweights(mgc_handle h, int axis, double* out);
int mgc_get_tweights(mgc_handle h, double* out);
/* weight of the arc (p, p + offset) for every voxel p (handle shape), NaN where p + offset is outside; offset has
 * ndim components in {-1,0,1}.  The read-back used for the full (8 / 26) neighbourhood. */
int mgc_get_nweights_offset(mgc_handle h, const int* offset, double* out);
int mgc_get_edge(mgc_handle h, int64_t i, int64_t j, double* out); /* Graph::get_edge, graph.h:482-498 */

/* Replaces GraphDouble.maxflow() (maxflow.cpp:472-604).  flow = capacity of the minimum cut
 * found (equals the reference's return value up to summation order, ~1e-12 relative). */
int mgc_maxflow(mgc_handle h, double* flow);

/* Replaces the per-voxel what_segment loop of bin/medpy_graphcut_voxel.py:177-181:
 * out[i] = 0 if SINK == what_segment(i) else 1. */
int mgc_labels(mgc_handle h, uint8_t* out);

/* The other side of the answer.  mgc_labels reports R_t, the voxels that can reach the sink in the residual graph of the
 * maximum flow (out = 0).  mgc_cut_sets computes, on the device, R_s = the voxels the source can reach in that residual graph --
 * the source side of the SMALLEST minimum cut, where mgc_labels' 1s are the source side of the largest -- and the AMBIGUITY SET
 * V \ (R_s u R_t): the voxels that some minimum cut puts on the source side and another on the sink side.  The minimum cut is unique
 * iff that set is empty.  from_source[i] / ambiguous[i] = 0 / 1 per voxel in C order; either pointer may be NULL (both: only the
 * counts are computed, nothing of the size of the volume comes down).  The sets are those of the handle's own residual graph with an
 * arc open where its residual capacity is > 0, no tolerance: exact on inputs whose arithmetic is exact (small integers), and on
 * floating-point inputs as fine-grained as the solve's own rounding.
 *   Valid on a single handle whose last mgc_maxflow converged, with no update or edit since (cold and warm solves, either
 * neighbourhood, whatever the capacities came from).  MGC_ERR_STATE before mgc_build, before mgc_maxflow, after an update or edit
 * that has not been solved, after MGC_ERR_NOT_CONVERGED and after mgc_finish; MGC_ERR_UNSUPPORTED on a slab handle; both before
 * anything is written.  A call leaves labels, label snapshot (mgc_labels_delta), residual state, statistics and launch counts of the
 * solve as they were; its mark planes come from the library's pool and go back, device_bytes is the same before and after.
 *   mgc_get_cut_sets_info, of the last mgc_cut_sets: out8 = {voxels from_source, voxels to_sink, voxels ambiguous, flood passes that
 * had tiles to visit, tile visits, tiles seeded (they hold excess), tiles skipped unread as wholly on the sink side, 0};
 * *source_cut = the capacity of the cut (R_s | V \ R_s), flow constant included -- a second minimum cut, so the value
 * mgc_maxflow returned (bit for bit where the arithmetic is exact, else up to the order of summation).  Either pointer may be NULL.
 * After a mgc_cut_sets that went through, mgc_last_error holds a note of where its time went (device_ms, download_ms). */
int mgc_cut_sets(mgc_handle h, uint8_t* from_source, uint8_t* ambiguous);
int mgc_get_cut_sets_info(mgc_handle h, int64_t* out8, double* source_cut);

/* The same three sets at a ROUNDING TOLERANCE.  On floating-point inputs a residual of a few ulp, or of DBL_MIN next to
 * weights of order 1, is open under one order of the solve's additions and 0.0 under another; mgc_cut_sets_tol judges every residual
 * against the size of the numbers it came from.  With scale(v) = the largest rcap(u -> w) + rcap(w -> u) over the arc pairs at v (both
 * ends voxels of the volume), an arc u -> v is open iff rcap > 0 and rcap > tol * max(scale(u), scale(v)); v is a source seed iff its
 * excess is > tol * max(|t-link as built|, scale(v)), a sink seed iff its residual sink link is.  from_source = what the source seeds
 * reach along open arcs, to_sink = what reaches a sink seed along them (a backward flood of its own: the labels are not consulted),
 * ambiguous = neither; 0 / 1 per voxel in C order, any of the three pointers may be NULL.  tol = 0 goes the same way and gives the sets
 * of mgc_cut_sets and the complement of mgc_labels; 64 * 2^-52 is the granularity the project's parity statement uses.
 *   States and refusals are those of mgc_cut_sets, checked before anything is written; MGC_ERR_INVALID for tol < 0, tol >= 1 or NaN.  A
 * call leaves labels, snapshot, residual state, statistics, launch counts and what mgc_get_cut_sets_info reports as they were, and
 * device_bytes the same.
 *   mgc_get_cut_sets_tol_info, of the last mgc_cut_sets_tol: out16 = {voxels from_source, to_sink, ambiguous; passes, tile visits, tiles
 * seeded of the forward flood; the same three of the backward flood; arcs with rcap > 0 that the threshold closed; t-links (excess > 0
 * or sink link > 0) that it closed; tiles the forward seeding skipped unread; 0, 0, 0, 0}; out4 = {tol, source_cut = capacity of the cut
 * around from_source, sink_cut = capacity of the cut around the complement of to_sink (flow constant included in both), the largest
 * scale(v)}.  Either pointer may be NULL.  mgc_last_error holds a note of where the time of the call went. */
int mgc_cut_sets_tol(mgc_handle h, double tol, uint8_t* from_source, uint8_t* to_sink, uint8_t* ambiguous);
int mgc_get_cut_sets_tol_info(mgc_handle h, int64_t* out16, double* out4);
int mgc_what_segment(mgc_handle h, int64_t i, int* segment); /* Graph::what_segment, graph.h:561-571 */

int mgc_get_node_num(mgc_handle h, int64_t* n);
int mgc_set_param(mgc_handle h, const char* name, int64_t value); /* solver schedule knobs: the table in DESIGN.md section 3 */
int mgc_get_stats(mgc_handle h, mgc_stats* out);
/* development aid (mgc_set_param "profile_sections" 1): out16[0..3] = shader cycles of workgroup lane 0 spent in
 * load+absorb / in-tile labels / push sweeps / store of k_discharge, out16[8..11] = how many such sections */
int mgc_get_profile(mgc_handle h, uint64_t* out16);
/* Which form of the solver kernels the last solve of the handle ran (mgc_maxflow, or the slab's part of mgc_solve_slabs): out[k] = launches
 * of kind k for k < min(n, MGC_NLAUNCH).  The parameters wave_kernels / use_filters / wave_min_tiles pick the form; the grid parameters
 * (grid26_dis, wave_grid_dis, wave_grid_rel, wave_grid26) size one form each, so a test of a grid can check that its kernel ran. */
enum {
    MGC_LAUNCH_DISCHARGE = 0,     /* k_discharge: one workgroup per tile (6-neighbourhood)                 */
    MGC_LAUNCH_DISCHARGE_W = 1,   /* k_discharge_w: one wave per tile, persistent grid wave_grid_dis      */
    MGC_LAUNCH_RELABEL_TILE = 2,  /* k_relabel_all / k_relabel_first_list / k_relabel_list / k_relabel_b  */
    MGC_LAUNCH_RELABEL_V = 3,     /* k_relabel_v                                                           */
    MGC_LAUNCH_RELABEL_W = 4,     /* k_relabel_w: one wave per tile, persistent grid wave_grid_rel        */
    MGC_LAUNCH_DISCHARGE26 = 5,   /* k26_discharge: grid grid26_dis (0: grid_cap)                         */
    MGC_LAUNCH_DISCHARGE26_V = 6, /* k26_discharge_v                                                       */
    MGC_LAUNCH_DISCHARGE26_W = 7, /* k26_discharge_w: one wave per tile, persistent grid wave_grid26      */
    MGC_LAUNCH_DT_AXIS = 8,       /* k_dt_axis: both scans of one axis of a distance transform            */
    MGC_LAUNCH_DT_SCAN = 9,       /* k_dt_scan: one scan of one axis (first_relabel_dt = 2, long lines, the z scans of a slab) */
    MGC_NLAUNCH = 10
};
int mgc_get_launch_counts(mgc_handle h, int64_t* out, int n);

/* ------------------------------------------------------------------------------------------
 * Z-slab decomposition across the GPUs of one node (no reference counterpart: the reference is
 * single-process; its only splitter, wrapper.py:72-204, is approximate and label-based).
 * One handle per slab.  The slab owns whole tile layers (8 voxel planes) of axis 0 and mirrors
 * one ghost tile layer per neighbour; mgc_set_* take the LOCAL sub-arrays (planes
 * info[0]..info[1] of the global arrays, ghost planes included).  The solve is mgc_solve_slabs (below): the single handle's
 * schedule with the packed borders (labels, outbox flow, suspect flags) exchanged at its hook points -- between the slabs' own
 * buffers when all slabs are handles of one process, over RCCL / xGMI inside the library (mgc_comm_init) when every rank holds
 * one, or through the caller's callbacks on host buffers (development transports).  mgc_solver_op / mgc_halo_pack / mgc_halo_unpack
 * issue single launches and single messages (profiling tools, the transport tests); no schedule is driven through them any more.
 * ---------------------------------------------------------------------------------------- */
enum {
    MGC_OP_ABSORB_ALL = 0,   /* -                                          */
    MGC_OP_FILL_INF = 1,     /* -                                          */
    MGC_OP_ZERO_COUNT = 2,   /* a0 = counter index                          */
    MGC_OP_RELABEL_ALL = 3,  /* a0 = next epoch, a1 = next list             */
    MGC_OP_RELABEL_LIST = 4, /* a0 = list, a1 = next epoch, a2 = next list  */
    MGC_OP_ACTIVATE = 5,     /* a0 = phase                                  */
    MGC_OP_DISCHARGE = 6,    /* a0 = list, a1 = phase, a2 = max cycles, a3 = max sweeps */
    MGC_OP_SUSPECT_PASS = 7, /* one pass of the tile-level suspect closure (sets counter MGC_CNT_CHANGED = 21 when something changed) */
    MGC_OP_RESET_SUSPECT = 8, /* a0 = next epoch, a1 = next list: suspect tiles -> labels INF, queued for relabelling */
    MGC_OP_FIRST_RELABEL = 9  /* the first global relabel of a solve by distance transform, on a single handle as built: a0 = 0 the transform towards
                                 the sink, 1 also the radial labels; a1 = c_min (radial_min_c).  MGC_ERR_STATE where the transform does not apply.
                                 Resets the launch counts; mgc_get_heights reads what it left. */
};
int mgc_create_slab(int ndim, const int64_t* global_shape, int connectivity, int device, int rank, int nranks, mgc_handle* out);
/* info[0..1] = local plane range [first, last) in the global volume (ghost planes included), info[2..3] = owned
 * plane range, info[4] / info[5] = has a lower / upper neighbour, info[6] = tiles per layer */
int mgc_slab_info(mgc_handle h, int64_t* info8);
int mgc_solver_op(mgc_handle h, int op, int64_t a0, int64_t a1, int64_t a2, int64_t a3);
int mgc_read_counts(mgc_handle h, int32_t* out32); /* 32 counters */
/* The distance labels of a single handle, one int32 per voxel in C order: which = 0 the array in use, 1 the one kept aside (the exact
 * labels while the radial ones are in use; MGC_ERR_STATE before there is one). */
int mgc_get_heights(mgc_handle h, int which, int32_t* out);
int mgc_halo_bytes(mgc_handle h, int kind, int64_t* bytes);
/* side 0 = lower / 1 = upper slab boundary; kind 0 = labels (relabel pass), 1 = labels + outbox flow (phase),
   2 = DIRTY / SUSPECT flags of the border tiles (suspect closure of an incremental relabel) */
int mgc_halo_pack(mgc_handle h, int side, int kind, void* buf, int buf_on_device);
int mgc_halo_unpack(mgc_handle h, int side, int kind, const void* buf, int buf_on_device, uint32_t epoch, int list);
/* after the slab driver has converged: labels of the local planes + this slab's part of the cut capacity */
int mgc_finish(mgc_handle h, double* flow_partial);

/* Native transport: RCCL over xGMI (librccl is dlopen()ed on first use, single-GPU users never need it).
 * Rank 0 obtains a 128-byte id (mgc_comm_unique_id) that the launcher broadcasts out of band (bench.py: a private directory of
 * files, medpy_amd/rendezvous.py -- no PyTorch anywhere in the package); every rank then calls mgc_comm_init on its slab handle.  mgc_halo_exchange =
 * pack both borders -> grouped ncclSend/ncclRecv with rank-1 / rank+1 -> unpack, all ordered on the handle's
 * stream (no host synchronisation).  mgc_allreduce_counts sums the 32 solver counters over all ranks
 * (ncclAllReduce) and returns them: the termination / fixpoint tests of the distributed schedule. */
int mgc_comm_unique_id(uint8_t* id128);
int mgc_comm_init(mgc_handle h, const uint8_t* id128);
int mgc_halo_exchange(mgc_handle h, int kind, uint32_t epoch, int list);

/* What a distributed solve did (global numbers; per-kernel times and this slab's own counts are in mgc_get_stats afterwards, as after
 * mgc_maxflow).  The host looks at the device only where every rank has to take the same decision (reduced counters). */
typedef struct mgc_slab_stats {
    int64_t outer;            /* global relabels                                            */
    int64_t relabel_passes;
    int64_t phases;           /* colour phases                                              */
    int64_t exchanges;        /* border exchanges (each ONE grouped send/receive per neighbour) */
    int64_t reductions;       /* counter all-reduces = points where the host waits for the device */
    int64_t converged;
    int64_t discharge_tiles;  /* global                                                     */
    int64_t relabel_tiles;    /* global                                                     */
    int64_t deferred_drains;  /* extra exchanges because a border message was full          */
    int64_t reserved[7];      /* [0]: cycles of colour phases that ran on radial labels */
} mgc_slab_stats;
int mgc_solve_slab(mgc_handle h, mgc_slab_stats* out);

/* ONE entry point for every way a volume's slabs can be laid out (round 6; the schedule is the single handle's own, mgc_solve in
 * medpy_amd/csrc/mgc_driver.inl, with the borders exchanged at its hook points -- first relabel by distance transform carried
 * across the slab borders, flood phase on radial labels, incremental relabels):
 *   n == the number of slabs of the volume: ALL slabs are handles of this process on one device (time-multiplexed on one GPU: how
 *       the multi-GPU schedule is exercised and measured where there is one GPU); `t` is ignored;
 *   n == 1, mgc_comm_init was called: this rank's slab, borders and reductions over RCCL / xGMI (what bench.py --gpus N runs);
 *   n == 1, `t` given: borders and reductions through the caller's callbacks on HOST buffers (development transports: gloo,
 *       a directory of files).
 * Replaces the serial loop of Graph::maxflow (maxflow.cpp:472-604) for a volume cut into Z-slabs. */
typedef struct mgc_transport {
    void* ctx;
    /* both borders at once: send_lo / recv_lo with rank - 1, send_hi / recv_hi with rank + 1 (a pair is NULL where the volume ends), nbytes each */
    int (*exchange)(void* ctx, const void* send_lo, void* recv_lo, const void* send_hi, void* recv_hi, int64_t nbytes);
    int (*allreduce)(void* ctx, int64_t* v, int n, int op); /* in place over all ranks; op 0 = sum, 1 = min */
    /* point to point with the neighbour on `side` (0: rank - 1, 1: rank + 1): the carry planes of the distance transforms, a pipeline over the ranks */
    int (*send)(void* ctx, int side, const void* buf, int64_t nbytes);
    int (*recv)(void* ctx, int side, void* buf, int64_t nbytes);
} mgc_transport;
int mgc_solve_slabs(mgc_handle* slabs, int n, const mgc_transport* t, mgc_slab_stats* out);
int mgc_allreduce_counts(mgc_handle h, int64_t* out32);


/* ======================================================================================
 * Sparse graphs ("msg"): everything that is not a 1-D..3-D voxel lattice -- the region graph of
 * graph_from_labels (reference medpy/graphcut/generate.py:177-338) with the terms of energy_label.py:33-404, voxel
 * graphs of more than three dimensions, and graphs assembled edge by edge through GCGraph.set_nweight
 * (graph.py:382-440).  One handle = one maxflow.GraphDouble (wrapper.cpp:59-89).
 * ==================================================================================== */
typedef struct msg_graph* msg_handle;

/* region terms, reference energy_label.py */
typedef enum msg_label_term {
    MSG_LABEL_STAWIASKI = 1,            /* energy_label.py:123-214; image = gradient image                         */
    MSG_LABEL_STAWIASKI_DIRECTED = 2,   /* energy_label.py:217-353; param = directedness (sign picks the direction) */
    MSG_LABEL_DIFFERENCE_OF_MEANS = 3   /* energy_label.py:33-120;  image = original image                          */
} msg_label_term;

typedef struct msg_stats {
    double  build_ms;        /* edge list -> CSR residual graph (sort, duplicate sums, reverse index) */
    double  solve_ms;
    int64_t rounds;          /* push + gather rounds                                               */
    int64_t global_relabels;
    int64_t relabel_passes;
    int64_t nodes;
    int64_t arcs;            /* distinct directed arcs                                             */
    int64_t edges_added;     /* sum_edge calls represented in the edge list                        */
    int64_t reserved[4];
} msg_stats;

/* GraphDouble(nodes, edges) + add_node(nodes) (graph.py:294-308, graph.cpp:12-31) */
int msg_create(int64_t nodes, int device, msg_handle* out);
int msg_destroy(msg_handle h);
const char* msg_last_error(msg_handle h);
int msg_set_param(msg_handle h, const char* name, int64_t value);

/* n calls of GCGraph.set_nweight(i, j, cap, rev) -> Graph::sum_edge (graph.py:382-440, graph.h:457-480): appended in
 * order, repeated (i, j) are added up in that order when the graph is solved */
int msg_add_edges(msg_handle h, int64_t n, const int64_t* i, const int64_t* j, const double* cap, const double* rev);
/* the n-links a voxel boundary term adds for an image of ANY number of axes (energy_voxel.py:611-664), generated
 * in HBM in the reference's order; term = mgc_term, spacing NULL = False */
int msg_add_lattice_edges(msg_handle h, int term, int ndim, const int64_t* shape, const void* image, int dtype, double sigma,
                          const double* spacing);
/* the n-links a region term adds for a label image with labels 1..nodes (energy_label.py); labels int64, C-order */
int msg_add_label_edges(msg_handle h, int term, int ndim, const int64_t* shape, const int64_t* labels, const void* image, int dtype,
                        double param);
/* per-region sums of `values` (and voxel counts) for labels 1..nregions: scipy.ndimage.mean / numpy.sum over a region
 * (energy_label.py:88, 394-397); accumulate_f32 = keep a float32 accumulator as numpy.sum does for float32 maps */
int msg_region_sums(int device, int64_t n, const int64_t* labels, const void* values, int dtype, int accumulate_f32, int64_t nregions,
                    double* sums, int64_t* counts);
/* merged t-links: tr[i] = tr_cap after all add_tweights calls, flow_const = what they added to the flow (graph.h:416-425) */
int msg_set_tweights_merged(msg_handle h, const double* tr, double flow_const);
/* Graph::maxflow may be called again after add_tweights and goes on from the residual graph it holds (lib/maxflow/src/
 * graph.h:129-132, 211-276).  Replaces the merged t-link of the n nodes ids[] (ids NULL: n == nodes, tr[] is the whole vector)
 * by tr[] and the flow constant by flow_const.  Checked before the first write -- ids in range, values finite, no id twice
 * (a list that does not ascend strictly is sorted in a copy) -- and a refused call (MGC_ERR_INVALID) leaves the handle as
 * it was.  On a handle that holds the residual graph of a finished solve (solved, no edges added since) the change is folded
 * into the resident excess / sink capacity of each node and the next solve is WARM: no CSR build, the push-relabel goes on
 * from the resident preflow.  The first such call after a solve keeps that solve's labels for msg_labels_delta.  On any
 * other handle (never solved, edges pending, last solve not converged, parameter "warm" = 0) only the t-links are stored
 * and the next solve is cold; that is no error. */
int msg_update_tweights(msg_handle h, int64_t n, const int64_t* ids, const double* tr, double flow_const);
/* after warm updates and the solve that followed: ascending ids of the nodes whose label differs from the solve before the
 * first of those updates.  *n = their number; more than cap: nothing is written.  MGC_ERR_STATE without such labels or
 * before the solve.  Same contract as mgc_labels_delta. */
int msg_labels_delta(msg_handle h, int64_t cap, int64_t* ids, int64_t* n);
/* out4: {the last solve skipped the CSR build, nodes folded by the last update, labels of an earlier solve are held,
 * cold builds on this handle so far} */
int msg_get_warm_info(msg_handle h, int64_t* out4);
/* GraphDouble.maxflow / what_segment / get_edge (pythongraph.h:20-21, graph.h:482-498, 561-571) */
int msg_maxflow(msg_handle h, double* flow);
int msg_labels(msg_handle h, uint8_t* out);
int msg_what_segment(msg_handle h, int64_t i, int* segment);
int msg_get_edge(msg_handle h, int64_t i, int64_t j, double* cap);
int msg_get_counts(msg_handle h, int64_t* nodes, int64_t* edges_added, int64_t* arcs);
/* every distinct arc of the graph as built (tail, head, capacity), sorted by (tail, head): bulk counterpart of get_edge,
 * used by the DIMACS writer (reference medpy/graphcut/write.py:29-76); arrays hold msg_get_counts(..., &arcs) entries */
int msg_get_arcs(msg_handle h, int32_t* tail, int32_t* head, double* cap);
/* The other side of the answer on a sparse graph: what mgc_cut_sets / mgc_cut_sets_tol compute for a voxel graph, over the
 * CSR arcs.  msg_labels reports R_t, the nodes that can reach the sink in the residual graph of the maximum flow (out = 0).
 * msg_cut_sets computes R_s = the nodes the source can reach there -- the source side of the SMALLEST minimum cut -- and the AMBIGUITY SET
 * V \ (R_s u R_t): the nodes some minimum cut puts on the source side and another on the sink side; the cut is unique iff that set is
 * empty.  An arc is open iff its residual capacity is > 0, no tolerance: exact where the arithmetic is exact (whole-number capacities).
 *   msg_cut_sets_tol judges every residual against the size of the numbers it came from.  With pair(a) = the capacities as built of arc a
 * and of its reverse arc added up, and scale(v) = the largest pair(a) over the arcs of v (0 without arcs), an arc u -> v is open iff
 * rcap > 0 and rcap > tol * max(scale(u), scale(v)); v is a source seed iff its excess is > 0 and > tol * max(|merged t-link|, scale(v)),
 * a sink seed iff its residual sink link is.  from_source = what the source seeds reach along open arcs, to_sink = what reaches a sink
 * seed along them (a backward flood of its own: the labels are not consulted), ambiguous = neither.  tol = 0 gives the sets of
 * msg_cut_sets and the complement of msg_labels; 64 * 2^-52 is the granularity the project's parity statement uses.
 *   Output: 0 / 1, one byte per node; any pointer may be NULL (all: only the counts are computed, nothing node-sized comes down).
 *   Valid on a handle whose last msg_maxflow converged, with no edges added and no msg_update_tweights / msg_set_tweights_merged since
 * (cold and warm solves alike).  MGC_ERR_STATE in any other state; MGC_ERR_INVALID for a NULL handle and for tol < 0, tol >= 1 or
 * NaN; all before anything is written.  A call leaves labels, the label snapshot of msg_labels_delta, the residual arrays, the flow,
 * msg_get_stats and msg_get_warm_info as they were; its planes are temporary and gone when it returns.
 *   msg_get_cut_sets_info, of the last call of either (MGC_ERR_STATE before the first): out16 = {nodes from_source, to_sink, ambiguous;
 * passes, seeds of the forward flood; passes, seeds of the backward flood; arcs with rcap > 0 that the threshold closed; t-links (excess
 * > 0 or sink link > 0) that it closed; 1 if the tol path ran; 0 ...}; out4 = {tol (-1 for the plain call), source_cut = capacity of
 * the cut around from_source, sink_cut = capacity of the cut around the complement of to_sink (the plain call: the flow msg_maxflow
 * returned), the largest scale(v) (0 for the plain call)}; the flow constant is included in both cuts, which equal the flow bit for bit
 * where the arithmetic is exact, else up to the order of summation.  Either pointer may be NULL.  After a call of msg_cut_sets /
 * msg_cut_sets_tol that went through, msg_last_error holds a note of where its device time went (device_ms, scale_ms, open_ms,
 * forward_ms, backward_ms, readout_ms). */
int msg_cut_sets(msg_handle h, uint8_t* from_source, uint8_t* ambiguous);
int msg_cut_sets_tol(msg_handle h, double tol, uint8_t* from_source, uint8_t* to_sink, uint8_t* ambiguous);
int msg_get_cut_sets_info(msg_handle h, int64_t* out16, double* out4);
int msg_get_stats(msg_handle h, msg_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* MEDPY_HIP_H */
