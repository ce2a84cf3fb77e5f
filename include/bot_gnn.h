/*
 * bot_gnn.h — C ABI of libbot_gnn.so: gfx950 (MI355X) message-passing kernels for full-batch
 * GAT / GCN forward + backward.
 *
 * This is the drop-in boundary.  Each entry point replaces one `dgl 0.5.*` operator that the
 * reference (AiRyunn/BoT) invokes from its layer code; the citation next to each function is the
 * reference call site (paths relative to the reference repository root).  The reference's own FFI
 * for this path is DGL's Python->C++ operator registry (`dgl.ops.gspmm / gsddmm / edge_softmax`,
 * reached through `graph.update_all`, `graph.apply_edges`, `dgl.ops.edge_softmax`); the host-side
 * binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless the name ends in `_host`.  The caller allocates and
 *    owns every buffer (inputs, outputs, workspace); the library never allocates, frees, copies,
 *    synchronises or keeps a pointer past the call — every launch function is hipGraph-capturable.
 *  - Work is enqueued on `stream` (a hipStream_t passed as void*) and NOT synchronised.
 *  - Return value: 0 = ok, < 0 = invalid argument (BOT_E_*), > 0 = a hipError_t from the launch.
 *    `bot_last_error()` returns a thread-local description of the last non-zero return.
 *  - A graph direction is given in compressed-row form: `indptr[n_rows+1]`, `indices[nnz]`.
 *    For the forward pass rows are DESTINATION nodes and indices are the SOURCE of every in-edge
 *    (CSC of the adjacency); for the transposed pass rows are sources and indices destinations.
 *    Within a row, positions are in ascending edge-id order.  Index type is int32.
 *  - "position order" = the order of `indices`; `perm[k]` maps position k to a row of an
 *    edge-indexed array (the edge id, or the position in the other direction).  NULL = identity.
 *  - Node features are fp32, laid out [n, H, D] with explicit strides in floats: `ld*` between
 *    nodes, `hs*` between heads (so padded layouts are allowed).  Edge arrays are [nnz, H] dense.
 *  - No float atomics anywhere: identical inputs give bitwise identical outputs run to run.
 */
#ifndef BOT_GNN_H
#define BOT_GNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BOT_ABI_VERSION 19

#define BOT_E_NULL (-1)     /* required pointer is NULL                 */
#define BOT_E_RANGE (-2)    /* size / stride / head count out of range  */
#define BOT_E_ALIGN (-3)    /* pointer not 4-byte aligned               */
#define BOT_E_PLAN (-4)     /* inconsistent row plan                    */

typedef void* bot_stream_t; /* hipStream_t */

int bot_abi_version(void);
const char* bot_last_error(void);
/* v17: a HIP stream of the library's own (hipStreamNonBlocking; high_priority != 0: the device's HIGHEST priority, 0: its LOWEST - not the
 * default priority torch's streams have: the side stream's workgroups are dispatched behind the main stream's when both have some ready,
 * which is what the step wants of work only the optimizer waits for, and what every A/B of bot_amd.side was measured with), never destroyed -
 * the second stream of bot_amd.side (weight-gradient products beside the sparse backward).  Not one of PyTorch's 32 pooled streams, which
 * are handed out round-robin and would sooner or later alias a capture stream or a process group's collective stream. */
int bot_stream_create(int32_t high_priority, bot_stream_t* out);
/* Name (as a profiler prints it) of the main device kernel the calling thread's most recent SpMM-family launch function
 * dispatched — the template instance depends on H, D and the operands' alignment.  Diagnostic only (bench.py names the
 * kernel of its roofline line from it); thread-local like bot_last_error. */
const char* bot_last_kernel(void);
/* v19, diagnostic only: from now on a SIGABRT / std::terminate in this PROCESS first appends the native frames of the thread that raised it
 * (and the uncaught exception's type and what()) to the file `path_host`, then runs the handler that was installed before (Python's
 * faulthandler) and ends the process as it would have ended.  abort() is raised on the calling thread, so the trace names the caller
 * (HIP runtime, RCCL watchdog, libstdc++).  tests/conftest.py arms it for every GPU test process; the product never calls it. */
int bot_debug_abort_trace(const char* path_host);

/* ---------------------------------------------------------------------------------------------
 * Row plan (host side, pure integer work; built once per graph direction).
 *
 * Splits rows longer than `chunk` neighbours into chunks so that no wavefront owns more than
 * `chunk` gathers (power-law tails), and lists those long rows.  A work item is 4 x int32:
 * {row, begin, end, slot}; slot < 0: the item owns the whole row and writes the result directly;
 * slot >= 0: the item writes a partial sum into workspace slot `slot`, and the long row's partials
 * [long_ptr[i], long_ptr[i+1]) are added in slot order afterwards (deterministic).
 * Items are emitted longest-first so heavy items start early.
 * ------------------------------------------------------------------------------------------- */
int bot_row_plan_size_host(const int32_t* indptr_host, int64_t n_rows, int32_t chunk,
                           int64_t* n_items, int64_t* n_long, int64_t* n_slots);
int bot_row_plan_fill_host(const int32_t* indptr_host, int64_t n_rows, int32_t chunk,
                           int32_t* items_host /* [n_items*4] */, int32_t* long_rows_host /* [n_long] */,
                           int32_t* long_ptr_host /* [n_long+1] */);
/* chunk size recommended for a graph with nnz edges (a quarter of one wavefront's share). */
int32_t bot_row_plan_default_chunk(int64_t nnz);

/* Row plan on the device (csrc/plan.hip): the arrays of bot_row_plan_size_host / bot_row_plan_fill_host, bit for bit, from a DEVICE
 * indptr (int32 [n_rows + 1]) - what a mini-batch graph is built with, so that nothing row-sized crosses to the host.  With
 * deg(r) = indptr[r+1] - indptr[r]: the long rows (deg > chunk) in ascending row order, row r cut into ceil(deg / chunk) items
 * {r, b, min(b + chunk, end), slot}, slot counting from 0 across all long rows, these items first; long_rows[k] = r, long_ptr[k] = the
 * first slot of the k-th long row, long_ptr[n_long] = n_slots; then one item {r, indptr[r], indptr[r+1], -1} per whole row (deg <= chunk,
 * 0 included), degree descending, stable in the row id.  n_items = n_rows - n_long + n_slots.
 *
 *   bot_row_plan_size_device   launches the sizing group and leaves sizes[0..2] = {n_long, n_slots, n_bad} (device int64 [3], every word
 *                              written), n_bad = the rows with indptr[r+1] < indptr[r] (the host planner's BOT_E_PLAN; the caller reads the
 *                              three words - its one device->host read - and does not fill when n_bad != 0).  It also sorts the rows into
 *                              `workspace` (bot_row_plan_device_workspace_bytes(n_rows) bytes, 8-byte aligned; -1 for n_rows out of range).
 *   bot_row_plan_fill_device   takes the same indptr / n_rows / chunk / workspace (untouched in between) and the three sizes, and writes
 *                              items [n_items, 4] (16-byte aligned), long_rows [n_long], long_ptr [n_long + 1].
 *
 * Integer arithmetic only and no atomic decides a position: the arrays are a pure function of indptr for every launch shape.  A fixed
 * number of launches (at most 8 + 3), none of which waits for another workgroup; a hub row is cut by one lane per item, not walked by one.
 * Argument checks, before any launch, with the host planner's codes: NULL indptr / sizes / outputs (workspace for n_rows > 0) ->
 * BOT_E_NULL; n_rows < 0 or >= 2^31 - 1, chunk < 1, a workspace too small -> BOT_E_RANGE; chunk > 1024 -> BOT_E_RANGE (the device
 * planner's own bound: bot_row_plan_default_chunk gives 64 .. 512; above it use the host planner); sizes that cannot belong to one plan
 * of n_rows rows -> BOT_E_PLAN.  n_rows == 0 -> 0, nothing launched (the empty plan: no items, long_ptr = {0}). */
int64_t bot_row_plan_device_workspace_bytes(int64_t n_rows);
int bot_row_plan_size_device(const int32_t* indptr, int64_t n_rows, int32_t chunk, void* workspace, int64_t workspace_bytes,
                             int64_t* sizes /* device [3] */, bot_stream_t stream);
int bot_row_plan_fill_device(const int32_t* indptr, int64_t n_rows, int32_t chunk, const void* workspace, int64_t workspace_bytes,
                             int64_t n_items, int64_t n_long, int64_t n_slots, int32_t* items /* [n_items*4] */,
                             int32_t* long_rows /* [n_long] */, int32_t* long_ptr /* [n_long+1] */, bot_stream_t stream);

/* Transpose of a finished CSC on the device (csrc/plan.hip): indptr int32 [n_dst + 1], indices int32 [nnz] (the source of each position,
 * in [0, n_src)) -> the CSR direction exactly as graph.build_direction compresses the same edges by source: indptr_r int32 [n_src + 1],
 * indices_r int32 [nnz] = the destination row of each entry, eid_r int32 [nnz] = its CSC position; inside a source row the entries
 * ascend in CSC position (a stable sort by source id).  Where the edge id IS the CSC position (a mini-batch graph), eid_r is also
 * csr2csc.  *n_bad (device int64, zeroed here) counts the indices outside [0, n_src); the other outputs are then undefined (but every
 * access stays in bounds).  workspace: bot_csc_transpose_workspace_bytes(nnz) bytes, 8-byte aligned (-1 for nnz out of range).
 * A stable LSD radix sort, 8 bits of the source id per pass: 2 + 3 * ceil(bits(n_src - 1) / 8) + 1 launches; integer work, no atomic
 * decides a position.  nnz == 0 -> 0, nothing launched: indptr_r stays the caller's zeros, *n_bad is not written (indices / indices_r /
 * eid_r / workspace may be NULL).  NULL pointers -> BOT_E_NULL; nnz, n_src or n_dst negative or >= 2^31 - 1, entries without rows, a small workspace -> BOT_E_RANGE. */
int64_t bot_csc_transpose_workspace_bytes(int64_t nnz);
int bot_csc_transpose_i32(const int32_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, int64_t nnz, int32_t* indptr_r,
                          int32_t* indices_r, int32_t* eid_r, int64_t* n_bad, void* workspace, int64_t workspace_bytes,
                          bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Degrees.  Replaces graph.in_degrees() / graph.out_degrees()
 * (src/no-sampling/models.py:335,352,388,478,501,551; src/ogbn-proteins/gat.py:64).
 * deg[r] = indptr[r+1] - indptr[r], int64, bit-exact.
 * ------------------------------------------------------------------------------------------- */
int bot_degrees_i64(const int32_t* indptr, int64_t n_rows, int64_t* deg, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SpMM.  Replaces update_all(fn.copy_src/copy_u, fn.sum)   — copy_u_sum  (models.py:374,381)
 *        and      update_all(fn.u_mul_e, fn.sum)            — u_mul_e_sum (models.py:547,
 *        src/ogbn-proteins/models.py:146, src/ogbn-products/models.py:147), and serves as their
 *        backward on the transposed direction.
 *
 *   out[r,h,:] = sum_{k in row r} w[wperm[k],h] * x[indices[k],h,:]  (+ addend[r,h,:])     (w == NULL: weight 1)
 *
 * `addend` (may be NULL; strides lda/hsa) is the fused epilogue for the layer's residual branch
 * `rst = rst + res_fc(h)` (models.py:558-560).  `partial` is caller-provided workspace of bot_spmm_workspace_floats(...) floats (may be NULL when
 * the plan has no long rows).
 * ------------------------------------------------------------------------------------------- */
int64_t bot_spmm_workspace_floats(int64_t n_slots, int32_t H, int32_t D);
/* Layout hint for the calling thread's following bot_spmm_f32 calls on weighted multi-head slabs whose head width is not a multiple
 * of 4 floats (3 x 250) and whose rows are H*D contiguous floats on a 16-byte aligned pitch >= H*D rounded up to x4: 0 (default) =
 * head-segment lanes with 8-byte loads, 1 = flat 16-byte lanes (spmm_flat_kernel).  Results are bitwise identical; flat is faster when
 * the gathered rows are L2-resident (graphs numbered for locality), slightly slower when they are fabric-bound.  Speed only. */
int bot_spmm_set_layout(int32_t layout);
/* Zero-weight skip of the weighted sweeps (bot_spmm_f32 with w, bot_spmm_dot_f32, bot_spmm_dot_halves_f16; not the flat layout, the
 * bcast forms or the blocked kernel), for the whole process: 1 (default) = an (entry, head) whose weight w[wperm[k],h] is exactly 0 - an
 * attention weight that dropout zeroed - issues no loads of x[indices[k],h,:]; its values count as 0, and the fused backward stores
 * dot_out[wperm[k],h] = 0.f instead of the dot product (its consumer, bot_gat_attn_bwd_f32, multiplies that entry by the same zero keep
 * factor).  0 = every row is read and every dot product computed.  On finite data `out` is the same bit for bit either way, and so is
 * dot_out wherever the weight is not 0.  With 1, a NaN / Inf in a slab reached only through zero weights no longer reaches the results,
 * and a caller that needs the gradient of a weight that is exactly 0 has to switch it off.  Anything but 0 / 1 -> BOT_E_RANGE. */
int bot_spmm_set_zero_skip(int32_t on);
int bot_spmm_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                 const int32_t* items, int64_t n_items,
                 const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long,
                 const float* x, int64_t ldx, int64_t hsx,
                 const float* w, const int32_t* wperm,
                 int32_t H, int32_t D,
                 float* out, int64_t ldo, int64_t hso,
                 const float* addend, int64_t lda, int64_t hsa,
                 float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * L2-blocked SpMM for dense graphs (mean degree in the hundreds).  Same result as bot_spmm_f32 (w in position order, no
 * addend) for the destination rows listed in `tile_rows`; other rows of `out` are not touched (the caller runs hub rows
 * through bot_spmm_f32 with a plan restricted to them).  The blocked edge structure is built once per graph direction
 * by the host (bot_amd/blocked.py): destination rows grouped into tiles of T (32/64/128/256) rows, sources cut into `nblk`
 * column blocks of `block_rows` (a power of two) rows, edges sorted by (tile, wave = slot % 16, block, slot, position):
 *   tile_rows[n_tiles*T]      destination row of each tile slot (-1: padding)
 *   ptr[n_tiles*16 + 1]       offsets of each wave's edge stream, (tile, wave)-major; a stream is sorted by (block, slot, position)
 *   b_src / b_lrow / b_pos    per blocked edge: source row, tile slot of its destination, position in the unblocked order
 * Rows of at most 32 (16) vector lanes are gathered `epi` = 2 (4) edges per instruction, one per 32- (16-) lane group; the
 * host then pads every (slot, block) run of a stream to a multiple of `epi` entries with b_src = -1 (no edge), streams
 * start at multiples of `epi`, and T may be 256.  epi = 1 otherwise.
 * One 1024-thread workgroup owns a tile and keeps its T output rows in LDS; its 16 waves cross the column blocks in
 * lockstep and all workgroups walk the blocks in the same order, so the block being gathered is resident in the XCD's L2; tiles are launched `round_tiles` at a time (one resident wave
 * of workgroups per launch).  H*D <= 1024 floats, T*H*D*4 <= 160 KB.  Rows are [H*D] contiguous with row strides ldx / ldo
 * (/ lda); `addend` (may be NULL) is the same residual epilogue as in bot_spmm_f32.  Deterministic, no atomics.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_blocked_f32(const int32_t* tile_rows, const int32_t* ptr, const int32_t* b_src, const uint8_t* b_lrow,
                         const int32_t* b_pos, int32_t n_tiles, int32_t nblk, int32_t block_rows, int32_t T, int32_t epi,
                         int32_t round_tiles, const float* x, int64_t ldx, const float* w, int32_t H, int32_t D, float* out,
                         int64_t ldo, const float* addend, int64_t lda, bot_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * Fused backward of u_mul_e_sum (models.py:547) in ONE sweep over the transposed direction (rows = sources u,
 * indices = destinations v): every gathered row x[v,h,:] (the upstream gradient) is used twice,
 *
 *   out[u,h,:]          = sum_{k in row u} w[wperm[k],h] * x[indices[k],h,:]      (gradient of the node features)
 *   dot_out[wperm[k],h] = < y[u,h,:] , x[indices[k],h,:] >                        (gradient of the edge weights)
 *
 * so a GAT layer's backward needs one E*H*D gather instead of the two of bot_spmm_f32 + bot_sddmm_dot_f32.
 * y is the layer's forward input slab (row-local).  D <= 1024 (16-byte aligned slabs) / 512 / 256.
 * absmax_slots (optional, NULL = off): max|out| is folded into these bot_absmax_slots() words as a by-product (see
 * "Maxima as by-products" below) — `out` then needs no separate pass before it becomes a halves-GEMM operand.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_dot_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                     const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long,
                     const float* x, int64_t ldx, int64_t hsx,
                     const float* w, const int32_t* wperm,
                     const float* y, int64_t ldy, int64_t hsy,
                     int32_t H, int32_t D,
                     float* out, int64_t ldo, int64_t hso,
                     float* dot_out, float* partial, uint32_t* absmax_slots, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Aggregate-before-project forms of u_mul_e_sum (models.py:547) for layers whose input is narrower than H*D — the
 * reordering GraphConv already applies for in_feats <= out_feats (models.py:377-385), valid for GAT because the
 * aggregation is linear:  sum_e a[e,h] (W_h x[u]) = W_h (sum_e a[e,h] x[u]).  The source row has no head axis and is
 * gathered once per edge for all H <= 4 heads (D <= 1024):
 *
 *   bot_spmm_bcast_f32       out[r,h,:] = sum_{k in row r} w[wperm[k],h] * x[indices[k],:]            x: [n_src, D]
 *   bot_spmm_dot_bcast_f32   out[r,:]   = sum_{k in row r} sum_h w[wperm[k],h] * x[indices[k],h,:]    x: [n, H, D] (ldx, hsx)
 *                            dot_out[wperm[k],h] = < y[r,:] , x[indices[k],h,:] >                     y: [n_rows, D]
 *
 * The second is the backward of the first on the transposed direction (x = gradient of the aggregated slab, y = the
 * layer input).  `out` of the first may be head-outer ([H, n, D]: hso = n*D, ldo = D) — the layout batched GEMMs want.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_bcast_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                       const int32_t* items, int64_t n_items,
                       const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long,
                       const float* x, int64_t ldx, const float* w, const int32_t* wperm,
                       int32_t H, int32_t D, float* out, int64_t ldo, int64_t hso,
                       float* partial, bot_stream_t stream);
/* v16: bot_spmm_bcast_f32 with the result written as a halves GEMM operand instead of fp32 (the aggregated slab's only consumers are the
 * per-head projection and its weight gradient, csrc/halves3.hip grouped forms): hout[r, h hsh + e] = h1, hout[r, h hsh + e + h2_off] =
 * 2^11 h2 of hscale[0] * out[r,h,e]  (halves_split's order 2), e < D; zeros for D <= e < hpiece.  hpiece, hsh, h2_off, ldh multiples of 4;
 * h2_off >= (H - 1) hsh + hpiece.  hscale: a device (s, 1/s) pair that bounds the result (sum_e w <= 1 per row: the scale of x does). */
int bot_spmm_bcast_halves_f16(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                              const int32_t* items, int64_t n_items,
                              const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long,
                              const float* x, int64_t ldx, const float* w, const int32_t* wperm,
                              int32_t H, int32_t D, const float* hscale, uint16_t* hout, int64_t ldh, int64_t hsh, int32_t h2_off,
                              int32_t hpiece, float* partial, bot_stream_t stream);
int bot_spmm_dot_bcast_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                           const int32_t* items, int64_t n_items,
                           const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long,
                           const float* x, int64_t ldx, int64_t hsx, const float* w, const int32_t* wperm,
                           const float* y, int64_t ldy, int32_t H, int32_t D,
                           float* out, int64_t ldo, float* dot_out, float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SDDMM dot.  The backward of u_mul_e_sum with respect to the edge weights (models.py:547):
 *
 *   out[operm[k], h] = < x[indices[k],h,:] , y[r,h,:] >        for every position k of every row r
 *
 * `accumulate` != 0 adds into `out` (used to tile D > the per-launch limit of 1024 floats).
 * ------------------------------------------------------------------------------------------- */
int bot_sddmm_dot_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                      const int32_t* items, int64_t n_items,
                      const float* x, int64_t ldx, int64_t hsx,
                      const float* y, int64_t ldy, int64_t hsy,
                      int32_t H, int32_t D,
                      float* out, const int32_t* operm, int32_t accumulate, bot_stream_t stream);

/* The same gradient for the aggregate-before-project layer (bot_spmm_bcast_f32) when its input needs no gradient (the first
 * layer of a stack): the source row has no head axis and is gathered once per edge for all H <= 4 heads,
 *
 *   out[operm[k], h] = < x[indices[k],:] , y[r,h,:] >          x: [n_src, D] (ldx);  y: [n_rows, H, D] (ldy, hsy; may be head-outer)
 *
 * 4*D gathered bytes per edge instead of the 4*H*D of bot_spmm_dot_bcast_f32, and no transposed sweep.  D <= 1024 / 512 / 256. */
int bot_sddmm_dot_bcast_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                            const int32_t* items, int64_t n_items,
                            const float* x, int64_t ldx,
                            const float* y, int64_t ldy, int64_t hsy,
                            int32_t H, int32_t D,
                            float* out, const int32_t* operm, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SDDMM copy_u / u_add_v.  Replaces apply_edges(fn.copy_u) / apply_edges(fn.u_add_v)
 * (models.py:525 / :523; proteins models.py:127 / :125) on the COO list in edge-id order:
 *
 *   out[e, :] = x[src[e], :] (+ y[dst[e], :] when y != NULL)          width W floats per node
 * ------------------------------------------------------------------------------------------- */
int bot_sddmm_u_add_v_f32(const int32_t* src, const int32_t* dst, int64_t n_edges,
                          const float* x, const float* y, int32_t W, float* out, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Attention logits + leaky-ReLU + per-destination softmax in one sweep (models.py:517-544):
 *
 *   z[k,h] = el[indices[k],h] (+ er[r,h]) (+ ee[eperm[k],h])        el, er: [n,H]; ee: [nnz,H]
 *   a[k,h] = softmax over the positions k of row r of leaky_relu(z[k,h], slope)
 *
 * `keep` (uint8, indexed through eperm like ee; may be NULL) restates the edge-drop branch
 * models.py:528-539: positions with keep == 0 are left out of the softmax and get a = 0.
 * With el == er == NULL, slope == 1 this is dgl.ops.edge_softmax(graph, ee) (models.py:544) on
 * logits given in edge-id order.  `a` is written at aperm[k] (NULL: position order).
 * `long_rows` (rows longer than the plan's chunk) are handled by one workgroup each.
 * `zsign` (may be NULL; H <= 8): uint8 [nnz], addressed like `a`; bit h receives [z > 0], so that the backward can take the
 * leaky-ReLU derivative from one byte per edge instead of re-gathering el[src] and re-reading ee.
 * `attn_drop` > 0 with `a_drop` [nnz,H] (addressed like `a`): the dropout behind the softmax (`self.attn_drop(...)`, models.py:544)
 * fused in — a_drop = a * keep / (1 - attn_drop), keep from a Philox4x32-10 stream keyed by (drop_seed [+ *seed_offset *
 * 0x9E3779B97F4A7C15], record index, head / 4); `a` itself stays the plain softmax (the backward needs it).  The backward
 * takes the gradient of a_drop in `da` with the same (attn_drop, drop_seed, seed_offset) and regenerates the mask.
 * Non-finite logits: a -inf logit is a dropped edge (a = 0, the rest of the row is the softmax without it); a row and head with
 * nothing kept, or nothing but -inf, gives zeros (NOT the reference's NaN); a NaN or +inf logit makes every kept entry of its row
 * and head NaN and touches no other row or head.
 * ------------------------------------------------------------------------------------------- */
int bot_gat_attn_fwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                         const int32_t* long_rows, int64_t n_long, int32_t chunk,
                         const float* el, const float* er, const float* ee, const int32_t* eperm,
                         const uint8_t* keep, float slope, int32_t H,
                         float* a, const int32_t* aperm, uint8_t* zsign,
                         float attn_drop, uint64_t drop_seed, const uint64_t* seed_offset, float* a_drop,
                         bot_stream_t stream);

/* Backward of the above.  Given a (forward output) and da (gradient w.r.t. a), both addressed
 * through aperm like the forward output:
 *
 *   t[r,h]   = sum_k a*da ;  de = a*(da - t) ;  dz = de * (z > 0 ? 1 : slope)
 *   dz[k,h]  written at zperm[k] (NULL: position order) — it is the gradient of ee, and the edge
 *            values whose per-source sum is the gradient of el (bot_segment_sum_f32 on the other
 *            direction);
 *   der[r,h] = sum_k dz[k,h]       (written when der != NULL)
 *
 * With el == er == NULL, slope == 1 this is the backward of dgl.ops.edge_softmax.  `zsign` (may be NULL): the sign bits the
 * forward stored; when given, el / er / ee / eperm / indices are not read.
 */
int bot_gat_attn_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                         const int32_t* long_rows, int64_t n_long, int32_t chunk,
                         const float* el, const float* er, const float* ee, const int32_t* eperm,
                         float slope, int32_t H,
                         const float* a, const float* da, const int32_t* aperm,
                         float* dz, const int32_t* zperm, float* der, const uint8_t* zsign,
                         float attn_drop, uint64_t drop_seed, const uint64_t* seed_offset, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Inference-only GAT layer: what `evaluate()` (src/no-sampling/run.py:290-322) needs from a layer — logits,
 * leaky-ReLU, per-destination softmax (models.py:517-544), aggregation (models.py:547), residual (models.py:558-560), then the
 * stack's eval-mode BatchNorm / bias and ReLU (models.py:726-734) — in ONE sweep over the in-edges, with nothing edge-sized
 * and no pre-BatchNorm [n,H*D] tensor written:
 *
 *   z[k,h]     = el[indices[k]*ldel + h] (+ er[r*lder + h]) (+ ee[k*H + h]);   e = leaky_relu(z, slope)
 *   a[k,h]     = softmax over the positions k of row r of e[k,h]
 *   out[r,h,:] = act( (sum_k a[k,h] * ew[k] * x[indices[k],h,:] + addend[r,h,:]) * scale[h*D+:] + shift[h*D+:] )
 *
 * el / er are node arrays with a row stride (they may be columns of the projection GEMM's output); ee [nnz,H] and ew [nnz]
 * are in position order; er, ee, ew, addend, scale, shift may each be NULL; relu != 0 applies max(.,0).  el == NULL (then er
 * and ee must be NULL) drops the softmax: out = act((sum_k ew[k] x[indices[k]] + addend) * scale + shift), the GraphConv
 * aggregation with its degree normalisation folded into ew (models.py:351-395).  Rows without in-edges give act(addend*scale
 * + shift).  Long rows (row plan) take a (max, 1/sum) pass first and are combined in slot order; `workspace` holds
 * bot_gat_infer_workspace_floats(n_slots, H, D) floats (may be NULL without long rows).  D <= 1024 / 512 / 256 by alignment.
 * Deterministic, no atomics.  Same value as bot_gat_attn_fwd_f32 + bot_spmm_f32 up to fp32 rounding of the online softmax.
 * Non-finite logits: a -inf logit among finite ones is a dropped edge wherever it lies in the row; a NaN or +inf logit makes
 * its (row, head) NaN and touches no other; a non-empty (row, head) of nothing but -inf is NaN (the reference's 0 / 0).
 * ------------------------------------------------------------------------------------------- */
int64_t bot_gat_infer_workspace_floats(int64_t n_slots, int32_t H, int32_t D);
int bot_gat_infer_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                      const int32_t* items, int64_t n_items,
                      const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots,
                      const float* x, int64_t ldx, int64_t hsx,
                      const float* el, int64_t ldel, const float* er, int64_t lder,
                      const float* ee, const float* ew, float slope, int32_t H, int32_t D,
                      const float* addend, int64_t lda, int64_t hsa,
                      const float* scale, const float* shift, int32_t relu,
                      float* out, int64_t ldo, int64_t hso,
                      float* workspace, uint32_t* absmax_slots /* optional: max|out|, "Maxima as by-products" */, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Segment sum of edge values.  Replaces update_all(fn.copy_e, fn.sum) — copy_e_sum
 * (src/ogbn-proteins/gat.py:58) — and serves the backward of copy_u / u_add_v (models.py:523,525):
 *
 *   out[r, :] = sum_{k in row r} vals[perm[k], :]                      width W floats per edge
 * ------------------------------------------------------------------------------------------- */
int bot_segment_sum_f32(const int32_t* indptr, int64_t n_rows, int64_t nnz,
                        const int32_t* long_rows, int64_t n_long, int32_t chunk,
                        const float* vals, const int32_t* perm, int32_t W,
                        float* out, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row gather / scatter-add used by the 1-D vertex-partitioned mode to pack halo rows for the RCCL
 * all-to-all and to fold received halo gradients back into owned rows (no reference counterpart:
 * the reference is single-device).  `rows` must be sorted-unique for the add form.
 *   gather:      out[i,:] = x[rows[i],:]
 *   scatter_add: x[rows[i],:] += vals[i,:]
 * ------------------------------------------------------------------------------------------- */
int bot_gather_rows_f32(const float* x, int64_t ldx, const int32_t* rows, int64_t n_sel, int32_t F,
                        float* out, int64_t ldo, bot_stream_t stream);
int bot_scatter_add_rows_f32(float* x, int64_t ldx, const int32_t* rows, int64_t n_sel, int32_t F,
                             const float* vals, int64_t ldv, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Hidden-layer epilogue: BatchNorm over the node axis + ReLU + dropout, fused.
 * Replaces `h = self.norms[i](h); h = self.activation(h); h = self.dropout(h)`
 * (src/no-sampling/models.py:636-639 and :726-731; nn.BatchNorm1d over ALL nodes, :609 / :698).
 *
 *   colstats      mean[c] = mean_r x[r,c];  m2[c] = sum_r (x[r,c]-mean[c])^2     (two-stage, fixed order)
 *   bn_act_fwd    y = drop_p( relu?( (x-mean)*invstd*weight + bias ) )
 *   bwd_reduce    g = dy * keep/(1-p) * [bn > 0];  sum_g[c] = sum_r g;  sum_gx[c] = sum_r g*xhat
 *   bwd_apply     dx = weight*invstd*( g - sum_g/count - xhat*sum_gx/count )
 *                 (sum_g == sum_gx == NULL: statistics were constants (eval mode): dx = weight*invstd*g)
 *
 * The dropout mask is a counter-based Philox4x32-10 stream: element (r, c) takes word c % 4 of the block with
 * counter r * ceil(F/4) + c/4 under key `seed` — a function of (seed, r, c, F) only, independent of pointer
 * alignment, strides or the vector width a launch picks, so forward and backward regenerate the same mask from
 * `seed` for any operand layout; nothing is stored.  `seed_offset` (device pointer, may be NULL): one 64-bit word read by
 * the kernel and mixed into the key (seed + word * 0x9E3779B97F4A7C15): a captured hipGraph bakes `seed` in, the caller
 * bumps the word between replays.  p == 0 disables dropout.  `weight`/`bias` may be
 * NULL.  `workspace` holds bot_bn_workspace_floats(F) floats.  In the vertex-partitioned mode the caller
 * all-reduces (mean, m2, count) and (sum_g, sum_gx) between the two halves; `total_count` is the global
 * row count.  The grad of weight is sum_gx, of bias sum_g.
 * ------------------------------------------------------------------------------------------- */
int64_t bot_bn_workspace_floats(int32_t F);
int bot_colstats_f32(const float* x, int64_t ldx, int64_t n, int32_t F, float* mean, float* m2, float* workspace,
                     bot_stream_t stream);
/* sum[c] = sum_r x[r,c], the same two-stage reduction without the pivot shift, finished in double: the bias gradient of the Linear /
 * GATConv bias over all N rows (src/no-sampling/models.py:548, src/ogbn-products/models.py:107, :262). */
int bot_colsum_f32(const float* x, int64_t ldx, int64_t n, int32_t F, float* sum, float* workspace, bot_stream_t stream);
/* colstats + everything nn.BatchNorm1d does with them in training mode, in one call: mean, invstd = rsqrt(m2/n + eps),
 * running_mean / running_var (may both be NULL) moved by `momentum` towards the batch mean / unbiased batch variance,
 * *num_batches_tracked (may be NULL) += 1.  Single-GPU form; the partitioned mode all-reduces between the two halves. */
int bot_bn_stats_f32(const float* x, int64_t ldx, int64_t n, int32_t F, float eps, float momentum, float* mean, float* invstd,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked, float* workspace,
                     bot_stream_t stream);
int bot_bn_act_fwd_f32(const float* x, int64_t ldx, int64_t n, int32_t F, const float* mean, const float* invstd,
                       const float* weight, const float* bias, int32_t relu, float p, uint64_t seed,
                       const uint64_t* seed_offset, float* y, int64_t ldy, bot_stream_t stream);
/* The same two calls when the epilogue's output is the next layer's GEMM operand (fp16 halves, see bot_gemm_halves_f32 below):
 * bn_stats_halves also tracks the column extremes and derives hscale = (s, 1/s) from the bound
 * max_c (|weight_c| max(|max_c - mean_c|, |min_c - mean_c|) invstd_c + |bias_c|) / (1 - p) >= max |y| — no pass over y;
 * bn_act_fwd_halves writes y AND its halves [h1 | h1 | 2^11 h2] (pieces of `piece` = F rounded up to x64 columns, zero padded; v15:
 * `pieces` = 2 leaves the duplicate out, [h1 | 2^11 h2] with ldh >= 2 * piece — halves_split's order 2), so the
 * separate halves_scale / halves_split passes over y disappear.  Needs the 4-column form (even F, 8-byte aligned rows).
 * y == NULL (v12): ONLY the halves are written — for a hidden state whose one consumer is the next projection GEMM (the backward
 * of this pass reads x, never y), which saves the fp32 store of an [n, F] matrix nobody reads. */
int bot_bn_stats_halves_f32(const float* x, int64_t ldx, int64_t n, int32_t F, float eps, float momentum, float* mean, float* invstd,
                            float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* weight,
                            const float* bias, float p, float* hscale, float* workspace, bot_stream_t stream);
int bot_bn_act_fwd_halves_f32(const float* x, int64_t ldx, int64_t n, int32_t F, const float* mean, const float* invstd,
                              const float* weight, const float* bias, int32_t relu, float p, uint64_t seed,
                              const uint64_t* seed_offset, float* y, int64_t ldy, const float* hscale, uint16_t* hout, int64_t ldh,
                              int32_t piece, int32_t pieces, bot_stream_t stream);   /* pieces: 3 = [h1 | h1 | 2^11 h2], 2 = [h1 | 2^11 h2] (v15) */
int bot_bn_act_bwd_reduce_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t n, int32_t F,
                              const float* mean, const float* invstd, const float* weight, const float* bias,
                              int32_t relu, float p, uint64_t seed, const uint64_t* seed_offset, float* sum_g, float* sum_gx,
                              float* workspace, bot_stream_t stream);
int bot_bn_act_bwd_apply_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t n, int32_t F,
                             const float* mean, const float* invstd, const float* weight, const float* bias,
                             int32_t relu, float p, uint64_t seed, const uint64_t* seed_offset, const float* sum_g,
                             const float* sum_gx, double total_count, float* dx, int64_t lddx, uint32_t* absmax_slots /* optional: max|dx|,
                             "Maxima as by-products" */, bot_stream_t stream);
/* v16: the BatchNorm backward WITHOUT a split pass behind it, for a dx whose only consumers are halves GEMMs (the aggregate-first GAT layer):
 *   bot_bn_act_bwd_reduce_max_f32   the reduce pass, which also leaves the column maxima of |g| and |xhat| in the workspace;
 *   bot_bn_bwd_bound_f32            max_c |w_c| invstd_c (max|g_c| + |sum_g_c| / n + max|xhat_c| |sum_gx_c| / n) >= max |dx| into by-product slots
 *                                   (sum_g / sum_gx: the FINAL sums, i.e. after a cross-rank reduction; NULL: eval statistics) — a scale
 *                                   for dx BEFORE dx exists (bot_halves_scale_from_slots_f32); a bound that is loose by a few binades costs
 *                                   nothing in this format (22 bits for entries down to 2^-28 of the scale);
 *   bot_bn_act_bwd_apply_halves_f32 the apply pass writing dx as a LEFT operand [h1 | 2^11 h2] (second half h2_off columns behind the first),
 *                                   columns in blocks of hD (a head; even, F % hD == 0) that start every hDP >= hD columns; the padding
 *                                   columns are NOT written (the caller zeroes them once); dx (fp32) may be NULL. */
int bot_bn_act_bwd_reduce_max_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t n, int32_t F,
                                  const float* mean, const float* invstd, const float* weight, const float* bias,
                                  int32_t relu, float p, uint64_t seed, const uint64_t* seed_offset, float* sum_g, float* sum_gx,
                                  float* workspace, bot_stream_t stream);
int bot_bn_bwd_bound_f32(int32_t F, int64_t n, const float* workspace, const float* sum_g, const float* sum_gx, double total_count,
                         const float* weight, const float* invstd, uint32_t* absmax_slots, bot_stream_t stream);
int bot_bn_act_bwd_apply_halves_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t n, int32_t F,
                                    const float* mean, const float* invstd, const float* weight, const float* bias,
                                    int32_t relu, float p, uint64_t seed, const uint64_t* seed_offset, const float* sum_g,
                                    const float* sum_gx, double total_count, float* dx, int64_t lddx, const float* hscale, uint16_t* hout,
                                    int64_t ldh, int32_t h2_off, int32_t hD, int32_t hDP, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Merged projection weight of a GAT layer (host-side convenience of the fused layer node, not a DGL operator): the layer's
 * linear maps on its input — fc (models.py:490-492), res_fc (:558-560), and the attention scores folded through fc,
 * el = h . (W_h^T attn_l[h]) (:517), er likewise (:521) — become ONE GEMM against
 *     merged [K, P] = [ W_fc^T (with_fc) | W_res^T (Wres != NULL) | wl | wr (attn_r != NULL) | 0 ... ]
 * with wl[k,h] = sum_d W_fc[h*D+d, k] * attn_l[h*D+d].  W, Wres: [H*D, K] row-major; attn_l, attn_r: [H*D].  `block` >= H*D is the
 * column width of each of the two copied blocks (zero padded): H*D rounded up to x4 puts the residual block of the GEMM output /
 * gradient buffer on a 16-byte boundary (3 x 250: columns [0, 750) | 2 pad | [752, 1502) | 2 pad | scores).  The backward takes
 * d merged and returns the gradients of the four parameters (dWres / d_attn_r NULL when absent).
 * ------------------------------------------------------------------------------------------- */
int bot_merge_weight_fwd_f32(const float* W, const float* Wres, const float* attn_l, const float* attn_r, int32_t H, int32_t D,
                             int32_t K, int32_t P, int32_t with_fc, int32_t block, float* merged, bot_stream_t stream);
int bot_merge_weight_bwd_f32(const float* W, const float* attn_l, const float* attn_r, int32_t H, int32_t D, int32_t K,
                             int32_t P, int32_t with_fc, int32_t block, const float* d_merged, float* dW, float* dWres,
                             float* d_attn_l, float* d_attn_r, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Edge-feature attention term of the ogbn-proteins GAT, fused.  Replaces, per layer,
 *   efeat_emb = relu(edge_encoder[i](efeat))                 src/ogbn-proteins/models.py:244-248
 *   attn_edge = attn_edge_fc(efeat_emb)                      src/ogbn-proteins/models.py:130-131
 * and their autograd:   ee[e,:] = W2 . relu(W1 . ef[e,:] + b1),   ef [E,I], W1 [J,I], b1 [J], W2 [H,J].
 * Only the reference's shape I = 8, J = 16 (H <= 8) is implemented (BOT_E_RANGE otherwise; callers fall back to
 * library ops).  `ef` and `ee`/`dz` are in the SAME edge order (the layers use CSC position order).  The backward
 * returns the three weight gradients (the edge features are inputs, not parameters); it runs the K = E reductions
 * on the fp32 MFMA and sums per-wavefront tiles in a fixed order.  workspace: bot_edge_mlp_workspace_floats().
 * ------------------------------------------------------------------------------------------- */
int64_t bot_edge_mlp_workspace_floats(void);
int bot_edge_mlp_fwd_f32(const float* ef, int32_t I, const float* W1, const float* b1, int32_t J, const float* W2,
                         int32_t H, int64_t n_edges, float* ee, bot_stream_t stream);
int bot_edge_mlp_bwd_f32(const float* ef, int32_t I, const float* W1, const float* b1, int32_t J, const float* W2,
                         int32_t H, const float* dz, int64_t n_edges, float* dW1, float* db1, float* dW2,
                         float* workspace, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training-time edge drop of the GAT layers.  Replaces
 *   perm = torch.randperm(graph.number_of_edges()); bound = int(E * edge_drop); eids = perm[bound:]
 *                                      src/no-sampling/models.py:528-532, src/ogbn-proteins/models.py:120-127
 * keep[e] = 1 for a uniformly random subset of exactly n_keep of the n edges, 0 for the others — the mask the
 * attention kernel takes (bot_gat_attn_fwd_f32 `keep`).  The subset is a pure function of (n, n_keep, seed): every
 * edge gets a 64-bit Philox4x32-10 key and the n - n_keep smallest keys are dropped, found by a radix select (no
 * sort, no n-sized temporary).  workspace: bot_random_keep_workspace_bytes() bytes, 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int64_t bot_random_keep_workspace_bytes(void);
int bot_random_keep_u8(int64_t n, int64_t n_keep, uint64_t seed, uint8_t* keep, void* workspace, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Neighbour sampling for mini-batch training (DGL's MultiLayerNeighborSampler, replace=False, and to_block, as
 * src/ogbn-products/gat.py:196-235 and src/ogbn-proteins/gat.py:174-200 use them).  Purely additive to ABI 19.
 *
 * count:  counts[i] = min(deg(seeds[i]), k) in-edges of seed i in the CSC (indptr [n_rows+1]); k < 0 = all in-edges.
 * sample: the chosen in-edges of seed i as CSC POSITIONS of the parent, ascending, into out[offsets[i] .. offsets[i+1]).
 *         Uniform without replacement (Floyd's algorithm, draw umulhi64(Philox4x32-10(seed, v << 32 | j), j + 1) for step j
 *         of row v); rows with deg <= k are copied whole.  A pure function of (graph, seeds, k, seed).  k <= 1024.
 * block:  the block's sources are the seeds in their order, then each newly reached node once in ascending parent id.
 *         `map` is int32 [n_nodes], all -1 between calls (and left so); tile_counts: bot_block_tiles(n_nodes) int64.
 *         mark:    seeds / reached sources into the map, *n_new (device) = the number of newly reached nodes.
 *         relabel: (after mark, n_src = n_seeds + *n_new) src_nid [n_src] parent ids, local[e] = block-local source of sampled
 *                  edge e (pos[e] a parent CSC position), parent_eid[e] = eid[pos[e]]; resets the touched map entries.
 * Argument checks: NULL pointers -> BOT_E_NULL, negative sizes / k > 1024 -> BOT_E_RANGE, no seeds -> 0 (nothing launched).
 * ------------------------------------------------------------------------------------------- */
int bot_sample_neighbors_count_i32(const int32_t* indptr, int64_t n_rows, const int32_t* seeds, int64_t n_seeds, int32_t k, int32_t* counts,
                                   bot_stream_t stream);
int bot_sample_neighbors_i32(const int32_t* indptr, int64_t n_rows, const int32_t* seeds, int64_t n_seeds, int32_t k, uint64_t seed,
                             const int64_t* offsets, int32_t* out, bot_stream_t stream);
int64_t bot_block_tiles(int64_t n_nodes);
int bot_block_mark_i32(const int32_t* seeds, int64_t n_seeds, const int32_t* indices, const int32_t* pos, int64_t n_pos, int32_t* map,
                       int64_t n_nodes, int64_t* tile_counts, int64_t* n_new, bot_stream_t stream);
int bot_block_relabel_i32(const int32_t* seeds, int64_t n_seeds, const int32_t* indices, const int32_t* eid, const int32_t* pos, int64_t n_pos,
                          int32_t* map, int64_t n_nodes, const int64_t* tile_offsets, int64_t n_src, int32_t* src_nid, int32_t* local,
                          int32_t* parent_eid, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Induced-subgraph extraction for partition / cluster mini-batches (Cluster-GCN; DGL's g.subgraph(nodes); csrc/subgraph.hip).
 * Purely additive to ABI 19.
 *
 * Input: the parent's CSC (indptr [n_rows+1], indices, eid; n_rows = n_nodes for the square parent this is for) and `nodes`,
 * n parent ids, UNIQUE, in the order they are to be numbered (local id = position in `nodes`).  `map` is the int32 [n_nodes]
 * table of the bot_block_* entry points: all -1 between calls, and left so after unmark.
 * Output: the CSC of the subgraph the set induces, rows = nodes in their order.  Row i holds the in-edges of nodes[i] whose source
 * is in the set, in the parent's CSC position order (stable): local_src[offsets[i] .. offsets[i+1]) = map[source], parent_eid =
 * eid[position].  The edge id of a subgraph edge is its CSC position, as in a block.
 *
 * mark:    map[nodes[i]] = i.  *n_dup (device) = the number of positions that lost their entry to another position, i.e. of
 *          duplicates (m positions naming one node: m - 1), plus 2^32 for every id outside [0, n_nodes) (never written to the
 *          map).  With *n_dup != 0 the set is not valid: unmark and stop.  An integer sum, independent of the execution order.
 * count:   counts[i] = the in-edges row i keeps.
 * fill:    (offsets = the exclusive scan of counts, offsets[n] = E_sub) local_src [E_sub], parent_eid [E_sub].
 * unmark:  map[nodes[i]] = -1.
 * One wavefront per row of at most 2048 in-edges (ballot + popcount, 256 positions in flight per wave); a longer row is swept by
 * a 1024-thread workgroup, 4096 positions per step, in the same order.  An id outside the parent's rows counts as an empty row.
 * No float arithmetic, no atomics on the structure: a pure function of (graph, nodes), bitwise reproducible.
 * Argument checks: NULL pointers -> BOT_E_NULL, negative sizes / n > n_nodes (n > n_rows) -> BOT_E_RANGE, n == 0 -> 0 (nothing
 * launched).
 *
 * tally (purely additive to ABI 19; GraphSAINT's aggregator normalisation, bot_amd/sampling.py saint_norms): after mark, for every
 *          listed node nodes[i] and every CSC position p of its row with map[indices[p]] >= 0 (the edges the set induces):
 *          tally[p] += 1.  tally: int32 [nnz], in CSC position order, the CALLER's accumulator (zeroed once, then one call per node
 *          set: tally[p] = the number of sets that induce the edge at p).  The traversal of count (one wavefront per row of at most
 *          2048 positions, a 1024-thread workgroup for a longer one); the lane that holds a kept position loads, adds and stores
 *          its own word.  Precondition, as for count / fill: the ids of `nodes` are unique - a position belongs to exactly one row
 *          and a row is listed once, so no word has two writers: no atomics, a pure function of (graph, node sets).
 *          Argument checks as count's: NULL indptr / map, and for n > 0 NULL indices / nodes / tally -> BOT_E_NULL; negative sizes,
 *          n > n_rows -> BOT_E_RANGE; n == 0 -> 0, nothing launched.
 * ------------------------------------------------------------------------------------------- */
int bot_subgraph_mark_i32(const int32_t* nodes, int64_t n, int32_t* map, int64_t n_nodes, int64_t* n_dup, bot_stream_t stream);
int bot_subgraph_count_i32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, const int32_t* nodes, int64_t n, const int32_t* map,
                           int32_t* counts, bot_stream_t stream);
int bot_subgraph_fill_i32(const int32_t* indptr, const int32_t* indices, const int32_t* eid, int64_t n_rows, const int32_t* nodes, int64_t n,
                          const int32_t* map, const int64_t* offsets, int32_t* local_src, int32_t* parent_eid, bot_stream_t stream);
int bot_subgraph_unmark_i32(const int32_t* nodes, int64_t n, int32_t* map, int64_t n_nodes, bot_stream_t stream);
int bot_subgraph_tally_i32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, const int32_t* nodes, int64_t n, const int32_t* map,
                           int32_t* tally, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GraphSAINT node sets for subgraph mini-batches (Zeng et al., ICLR 2020; DGL's SAINTSampler modes "walk" and "node"):
 * csrc/saint.hip (the walks) and csrc/sampling.hip (the node list, on the block builder's scan).  Purely additive to ABI 19.
 * The batch itself is bot_subgraph_*_i32 on the listed nodes.
 *
 * walk:   trace int32 [n_roots, length + 1], row i = walk i over the parent's CSC (indptr [n_rows + 1], indices [nnz]).
 *         The draw of walk i at step t is x(i, t) = the first 64 bits of Philox4x32-10(seed, counter = i << 32 | t) (word 0 the
 *         high half, as bot_sample_neighbors_i32 forms its draw); a value in [0, r) is umulhi64(x, r) (bias below 2^-32).
 *         Step 0, the root.  root_mode 0: nids[umulhi64(x, n_nids)], or umulhi64(x, n_rows) itself when nids is NULL - uniform,
 *         with replacement (GraphSAINT's random-walk sampler).  root_mode 1: indices[umulhi64(x, nnz)], the source of a uniformly
 *         drawn edge - a node drawn in proportion to its out-degree (GraphSAINT's node sampler; on a bidirected graph also its
 *         in-degree); nids must be NULL and nnz > 0.
 *         Step t = 1 .. length: from v to indices[indptr[v] + umulhi64(x, deg(v))], a uniformly drawn in-neighbour; deg(v) = 0
 *         stays at v.  The walk follows in-edges backwards: the node reached sends a message to the node it was reached from, so
 *         that edge is in the induced subgraph (on a bidirected graph this is DGL's random_walk distribution).
 *         A pure function of (graph, nids, n_roots, length, root_mode, seed): independent of the launch shape and of the run.  One
 *         lane per walk, one wave per workgroup; an id of `nids` outside [0, n_rows) is copied to its row of the trace and never
 *         used as an index.
 * nodes:  the distinct entries of `trace` (n_trace values) in ASCENDING id, through `map`, the int32 [n_nodes] table of the
 *         bot_block_* entry points (all -1 between calls, and left so); tile_counts: bot_block_tiles(n_nodes) int64.
 *         mark:  n_out[0] (device) = the number of distinct ids inside [0, n_nodes); n_out[1] += the number of entries outside that
 *                range, which are skipped (the CALLER zeroes n_out before the call; a trace of bot_saint_walk_i32 has none).
 *         list:  (after mark, n = n_out[0]) nodes int32 [n]; resets the touched map entries.
 *         Plain stores and integer arithmetic (every writer of a map entry stores the same value): deterministic.
 * Argument checks: NULL pointers -> BOT_E_NULL; negative sizes, n_roots (length + 1) >= 2^31, n_rows or nnz >= 2^31, a root_mode
 * other than 0 / 1, root_mode 1 with nids or with nnz = 0, roots asked of an empty node set, n > n_nodes -> BOT_E_RANGE; no roots /
 * an empty trace / n = 0 -> 0 (nothing launched).
 * ------------------------------------------------------------------------------------------- */
int bot_saint_walk_i32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* nids, int64_t n_nids,
                       int64_t n_roots, int32_t length, int32_t root_mode, uint64_t seed, int32_t* trace, bot_stream_t stream);
int bot_saint_nodes_mark_i32(const int32_t* trace, int64_t n_trace, int32_t* map, int64_t n_nodes, int64_t* tile_counts, int64_t* n_out,
                             bot_stream_t stream);
int bot_saint_nodes_list_i32(int32_t* map, int64_t n_nodes, const int64_t* tile_offsets, int64_t n, int32_t* nodes, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Exact multi-task ROC-AUC counts (OGB's Evaluator("ogbn-proteins"): the Mann-Whitney statistic of every task), csrc/rocauc.hip.
 * Purely additive to ABI 19.
 *
 * pred    float32 [n, T], row stride ldp >= T (in floats).
 * labels  int8 [n, T], row stride ldl >= T: 1 = positive, 0 = negative, anything else = not labelled, the entry is ignored.
 * groups  int8 [n] or NULL: g in [0, G) is the row's group (the train / validation / test split), any other value excludes the row;
 *         NULL puts every row into group 0.  1 <= G <= 8.
 * out     int64 [G, T, 3]: for group g and task t (n_pos, n_neg, 2U) over the counted entries of that (group, task), with
 *         2U = sum over its (positive p, negative q) pairs of 2 [s_q < s_p] + [s_q == s_p]; ROC-AUC = 2U / (2 n_pos n_neg).  Pairs are
 *         formed inside a group only.
 * Scores compare as IEEE float32 values: -0.0 equals +0.0, +-inf are ordinary ordered values, denormals are distinct values.  A NaN
 * in a counted entry is not ordered: such entries are left out of `out` and counted into nan_count[0] (int64, device), which the
 * caller turns into an error.  A NaN in an excluded row or an unlabelled entry is not counted.
 * Integer arithmetic and integer atomics only: `out` is a pure function of the inputs, the same for any launch shape and any run.
 * The entry point zeroes out and nan_count itself.  n = 0: nothing is launched and nothing written (the caller's zeros stay).
 * Method: task-major order-preserving uint32 keys + one code byte per entry; a stable least-significant-digit radix sort (4 passes
 * of 8 bits, tasks on grid.y, 4096 entries per workgroup, ranks inside a wave by __ballot); a sweep over 2048-entry tiles that adds,
 * per positive, the group's negatives in front of its tie run and through its end (tie runs followed across tiles by binary search).
 * Ranges (BOT_E_RANGE before any launch): 0 <= n < 2^31 (so 2U < 2^63 and positions fit uint32), 1 <= T <= 65535 (grid.y),
 * n T < 2^40 (the workspace is 10 n T bytes + tables), ldp / ldl >= T, 1 <= G <= 8, workspace_bytes >= bot_rocauc_workspace_bytes(n, T, G).
 * NULL out / nan_count, and for n > 0 NULL pred / labels / workspace -> BOT_E_NULL; workspace not 8-byte aligned -> BOT_E_ALIGN.
 * bot_rocauc_workspace_bytes: the bytes of `workspace` (non-decreasing in n, T and G), -1 outside the ranges above.
 * ------------------------------------------------------------------------------------------- */
int64_t bot_rocauc_workspace_bytes(int64_t n, int32_t T, int32_t G);
int bot_rocauc_f32(const float* pred, int64_t ldp, const int8_t* labels, int64_t ldl, const int8_t* groups, int64_t n, int32_t T, int32_t G,
                   int64_t* out, int64_t* nan_count, void* workspace, int64_t workspace_bytes, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Propagation step: one iteration of label propagation / Correct and Smooth (Huang et al., ICLR 2021; bot_amd/smoothing.py),
 * csrc/propagate.hip.  Purely additive to ABI 19.
 *
 * One sweep over the in-edges of a SQUARE direction (rows = destinations, indices < n_rows) with its row plan; for every row v and
 * column c < C:
 *   s          = sum_{k in row v} src_scale[indices[k]] * y[indices[k], c]        (src_scale NULL: 1)
 *   t          = alpha * dst_scale[v] * s + beta * y0[v, c]                       (dst_scale NULL: 1)
 *   out[v, c]  = fixed != NULL && fixed[v] ? y0[v, c] : min(max(t, lo), hi)       (lo = -inf, hi = +inf: no clamp; a NaN stays a NaN)
 *   row_abs[v] = sum_c |out[v, c]|                                                (row_abs NULL: not written)
 * With out_scale != NULL the row is STORED as out_scale[v] * out[v, :] (fixed rows and row_abs are those of the unscaled out): passing the
 * next sweep's src_scale here leaves the iterate pre-scaled, and that sweep runs with src_scale = NULL - no second random read per edge.
 * y, y0, out: float32 [n_rows, C] with row strides ldy / ldy0 / ldo >= C (in floats); src_scale, dst_scale, out_scale, row_abs: float32
 * [n_rows]; fixed: uint8 [n_rows].  `out` may be y0 but must not be y (other rows' sums read y while out is written).  A row without in-edges
 * has s = 0.  Rows longer than the plan's chunk are summed chunk by chunk into `partial` (n_slots * C floats; may be NULL when the
 * plan has no long rows) and combined in slot order, as in bot_spmm_f32.  16-byte lanes when C and the strides are multiples of 4
 * floats and the bases 16-byte aligned, 8-byte lanes for multiples of 2, else 4-byte lanes; rows of at most 8 / 16 / 32 lanes share
 * a wavefront, 8 / 4 / 2 destinations to one.  The row scale, the axpy, the clamp, the reset of fixed rows and the row norm are the
 * epilogue of the lanes that hold the row's sum: one launch per iteration (two with long rows).  No atomics; the bytes of out and
 * row_abs repeat from call to call.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, C outside 1..1024, a row stride below C, out == y -> BOT_E_RANGE;
 * n_rows = 0 -> 0, nothing launched; NULL items / y / y0 / out, NULL indices with nnz > 0, long rows without long_rows / long_ptr /
 * partial -> BOT_E_NULL; a pointer off its 4-byte (items: 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_propagate_step_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                           const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* y, int64_t ldy, const float* y0,
                           int64_t ldy0, float* out, int64_t ldo, int32_t C, float alpha, float beta, const float* src_scale,
                           const float* dst_scale, float lo, float hi, const uint8_t* fixed, float* row_abs, const float* out_scale,
                           float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The propagation step with edge weights (csrc/propagate.hip).  Purely additive to ABI 19.
 *
 * The operands, checks and results of bot_propagate_step_f32, plus ew: float32 [nnz], one weight per edge in CSC POSITION order
 * (4-byte aligned, else BOT_E_ALIGN).  The row's sum becomes
 *   s = sum_{k in row v} ew[k] * src_scale[indices[k]] * y[indices[k], c]
 * and everything behind the sum (dst_scale, the axpy, the clamp, fixed rows, row_abs, out_scale, long rows through `partial`) is the
 * unweighted step's.  ew[k] is read by the lane that reads indices[k] - both sequential - and multiplied into that lane's source
 * scale before it is broadcast, so the product per edge is fl(ew[k] * src_scale[u]) and ew = 1.0f everywhere gives the bytes of
 * bot_propagate_step_f32.  Weights are not checked (finite, non-negative ones are what bot_amd/smoothing.py's normalisations assume).
 * One more streamed 4-byte word per edge and sweep.  No atomics; the bytes repeat from call to call.
 * ew == NULL behaves exactly as bot_propagate_step_f32 (the same kernels).
 * ------------------------------------------------------------------------------------------- */
int bot_propagate_step_w_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* y, int64_t ldy, const float* y0,
                             int64_t ldy0, float* out, int64_t ldo, int32_t C, float alpha, float beta, const float* src_scale,
                             const float* dst_scale, float lo, float hi, const uint8_t* fixed, float* row_abs, const float* out_scale,
                             float* partial, const float* ew, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * APPNP step: one step of personalised-PageRank propagation, forward or backward, with edge dropout regenerated from a counter
 * (APPNP: Gasteiger et al., ICLR 2019; GCNII: Chen et al., ICML 2020; bot_amd/ops.py appnp_propagate), csrc/appnp.hip.  Purely
 * additive to ABI 19.
 *
 * One sweep over a SQUARE direction (indices < n_rows) with its row plan; for every row v and column c < C:
 *   q_k  = pos != NULL ? pos[k] : k                                        (the mask's index of position k)
 *   m_k  = p == 0 ? 1 : (keep(seed, step, q_k) ? 1 / (1 - p) : 0)
 *   f_k  = src_scale[indices[k]] (NULL: 1) * ew[k] (if given) * m_k (if p > 0)
 *   s    = sum_{k in row v} f_k * y[indices[k], c]                         (position order)
 *   o    = fma(a * dst_scale[v] (NULL: 1), s, b * y0[v, c])                (y0 NULL: o = a * dst_scale[v] * s)
 *   acc_out[v, c] = acc_in[v, c] + o                                       (only when acc_out != NULL; acc_in may be acc_out, or y)
 *   out[v, c]     = out_scale[v] (NULL: 1) * o
 * keep(seed, step, q) is word q & 3 of Philox4x32-10 under the 64-bit key `seed` at the counter ((uint64)step << 32) | (q >> 2); the
 * position is kept iff (w >> 8) * 2^-24 >= p.  The mask is a function of (seed, step, q) only, never of the lane layout: the forward
 * sweeps the CSC with pos = NULL, the backward the CSR with pos = the CSC position of every CSR position, and both see one mask per
 * (step, edge); parallel edges have positions and bits of their own.  A dropped position contributes nothing whatever its source row
 * or weight holds (NaN and inf included), and its source row is not gathered.
 * y, y0, out, acc_in, acc_out: float32 [n_rows, C] with row strides ldy / ldy0 / ldo / ld_acc_in / ld_acc_out >= C (in floats);
 * src_scale, dst_scale, out_scale: float32 [n_rows]; ew: float32 [nnz] and pos: int32 [nnz], both in the position order of the
 * direction swept.  `out` and `acc_out` must not be y (other rows' sums read y while they are written); out may be y0.  The
 * multiplications by absent operands do not happen: with p == 0, ew == NULL, pos == NULL, acc_out == NULL and y0 given, `out` is bit
 * for bit what bot_propagate_step_f32 stores with lo = -inf, hi = +inf, fixed = NULL, row_abs = NULL.  Long rows go chunk by chunk
 * through `partial` (n_slots * C floats) and are combined in slot order; lanes and lane groups as in bot_propagate_step_f32, the lane
 * width chosen over y, y0, out, acc_in, acc_out and partial.  No atomics: each element of acc is read and written by one lane, and the
 * bytes of out and acc_out repeat from call to call.
 * Bound per entry against exact arithmetic, mag = the sum of the absolute values of the entry's terms:
 * (deg + 8 + [ew] + [p > 0]) * 2^-24 * mag; acc_out adds 2^-24 * (|acc_in| + |o|).
 * HBM model per sweep: 4 * [E_kept * C + E * (1 + [src_scale] + [ew] + [pos]) + N * C * (1 + [y0] + 2 * [acc])] bytes.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, C outside 1..1024, p outside [0, 1), a negative step, a row
 * stride below C, out == y, acc_out == y -> BOT_E_RANGE; n_rows = 0 -> 0, nothing launched; NULL items / y / out, NULL indices with
 * nnz > 0, acc_out without acc_in, long rows without long_rows / long_ptr / partial -> BOT_E_NULL; a pointer off its 4-byte (items:
 * 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_appnp_step_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                       const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* y, int64_t ldy, const float* y0,
                       int64_t ldy0, float* out, int64_t ldo, int32_t C, float a, float b, const float* src_scale, const float* dst_scale,
                       const float* out_scale, const float* acc_in, int64_t ld_acc_in, float* acc_out, int64_t ld_acc_out, float* partial,
                       const float* ew, const int32_t* pos, float p, uint64_t seed, int32_t step, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Max aggregation (csrc/spmm_max.hip): the element-wise max over a row's neighbours with its argmax, and the backward that routes
 * the gradient to that one neighbour.  GraphSAGE's pool aggregator (Hamilton, Ying, Leskovec, NeurIPS 2017) and
 * update_all(fn.copy_u, fn.max).  Purely additive to ABI 19.
 *
 * Forward, over a direction with its row plan (rows = destinations): x float32 [n_src, F] (row stride ldx >= F, unit inner stride,
 * indices < n_src not checked), out float32 [n_rows, F] (ldo), arg int32 [n_rows, F] (lda).
 *   out[r, f] = max_k x[indices[k], f] over the positions k of row r;   arg[r, f] = the SMALLEST position k that attains it
 * (k indexes `indices`: the CSC position, not the source id, so parallel edges stay apart).  Ties are numeric (-0.0 == +0.0; the
 * earlier position wins).  An empty row gives out = 0, arg = -1.  relu != 0: out = max(m, 0) and arg = -1 wherever m <= 0
 * (max_u relu(z_u) = relu(max_u z_u): the ReLU in front of the reduce is never a pass of its own).  NaN inputs: the value at that
 * (row, column) is unspecified, arg is -1 or a position of the row, nothing faults.  Rows longer than the plan's chunk leave one
 * (max, position) pair per chunk in `workspace` (2 * n_slots * F 4-byte words, 16-byte aligned; may be NULL without long rows) and
 * are folded in slot order.  Lane layout as in bot_propagate_step_f32; rows wider than 128 lanes walk feature tiles.
 *
 * Backward, over the TRANSPOSED direction (rows = sources) with pos int32 [nnz] = the forward direction's position of each entry
 * (Graph.csr2csc): dout float32 and arg int32 are indexed by this direction's `indices` (the destinations), dx float32 [n_rows, F].
 *   dx[u, f] = sum_j (arg[indices[j], f] == pos[j] ? dout[indices[j], f] : 0) over the positions j of row u, in position order;
 * long rows chunk by chunk into `partial` (n_slots * F floats, 16-byte aligned) and added in slot order.
 *
 * No atomics; the bytes of out, arg and dx repeat from call to call.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, F < 1, a row stride below F, out == x / dx == dout -> BOT_E_RANGE;
 * n_rows = 0 -> 0, nothing launched; NULL items or operands, long rows without long_rows / long_ptr / workspace -> BOT_E_NULL; a
 * pointer off its 4-byte (items, workspace: 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_max_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* x, int64_t ldx, int32_t F,
                     int32_t relu, float* out, int64_t ldo, int32_t* arg, int64_t lda, void* workspace, bot_stream_t stream);
int bot_spmm_max_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                         const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const int32_t* pos, const float* dout, int64_t ldd,
                         const int32_t* arg, int64_t lda, int32_t F, float* dx, int64_t ldx, float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PNA aggregation (csrc/spmm_pna.hip): the aggregators of Principal Neighbourhood Aggregation (Corso, Cavalleri, Beaini, Lio,
 * Velickovic, NeurIPS 2020) - mean, sum, max, min, std, var - of ONE gather of the neighbours' rows, each times scalers of the
 * in-degree, and the backward.  bot_amd.nn.PNAConv, ops.pna_aggregate, update_all(fn.copy_u, fn.min).  Purely additive to ABI 19.
 *
 * Forward, over a direction with its row plan (rows = destinations): a float32 [n_src, F] (lda), b float32 [n_rows, F] (ldb) or NULL.
 * For row r with n > 0 positions k and m_k = a[indices[k]] + b[r], per column:
 *   mean = mean_k m_k, sum = sum_k m_k, max / min the extremes, var = relu(mean_k m_k^2 - mean^2), std = sqrt(var + 1e-30)
 * computed as mean = p + S1 / n, var = relu(S2 / n - (S1 / n)^2) from S1 = sum d_k, S2 = sum d_k^2, d_k = a[indices[k]] - p, with the
 * pivot p = the row of the first neighbour, a[indices[indptr[r]]] (pivot == 0: p = a[0], any row - for measurements), sums in position
 * order; a row of equal neighbours, or of one, has var = 0 exactly.  Max and min compare strictly in position order (the owner is
 * the smallest position that attains it, -0.0 == +0.0, a NaN never enters); sums carry a NaN.  aggs: a HOST array of A (1 .. 8) codes,
 * 0 mean, 1 sum, 2 max, 3 min, 4 std, 5 var; scale: DEVICE float32 [S, n_rows] (S 1 .. 8; NULL with S == 1: ones), the scalers.
 *   out[r, tower * S*A*Ft + (s*A + g) * Ft + f] = scale[s, r] * aggregator g at column tower * Ft + f      (out [n_rows, S*A*F], ldo)
 * Ft divides F.  A row without positions is all zeros (no b, whatever scale holds).  saved float32 [n_rows, 2 F] (lds; or NULL) takes
 * the mean of a (without b) and, in its second half, std where var > 0 and 0 where var == 0 (the backward's gate); sarg int32
 * [n_rows, 2 F] (ldg; NULL with saved) the positions of the max and of the min, -1 on an empty row.  Rows longer than the plan's chunk
 * leave (S1, S2, max, position, min, position) per chunk in `workspace` (6 * n_slots * F 4-byte words, 16-byte aligned; may be NULL
 * without long rows) - every chunk with the row's pivot - and are folded in slot order.  Lane layout as in bot_spmm_max_f32, the vector
 * width chosen so that Ft and every stride are multiples of it.
 *
 * bot_pna_bwd_prep_f32, a dense pass over [n_rows, F]: with G_g = sum_s scale[s, r] * dout[r, block (s, g)], writes db[r] (or NULL) =
 * the sum of G_g over mean, max, min and n G_g for sum, and one record of `sections` * F words per destination (rec, ldr), the
 * sections the aggregators need in the fixed order  g0 (mean: G / n, sum: G) | c1 (std: G / (n std), var: 2 G / n; 0 where var == 0) |
 * mean of a (with c1) | gmax | gmin | argmax | argmin (int32 bits).
 *
 * bot_spmm_pna_bwd_f32, over the TRANSPOSED direction (rows = sources) with pos int32 [nnz] (Graph.csr2csc), gathers one record per
 * out-edge:  dx[u] = sum_j g0[v_j] + c1[v_j] * (a[u] - mean[v_j]) + gmax[v_j] * (argmax[v_j] == pos[j]) + gmin[v_j] * (argmin[v_j] ==
 * pos[j]) in position order; long rows chunk by chunk into `partial` (n_slots * F floats, 16-byte aligned), added in slot order.  a
 * may be NULL without std / var.
 *
 * No atomics; the bytes of every output repeat from call to call.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, F < 1, Ft < 1 or F % Ft != 0, A or S outside 1 .. 8, an unknown
 * aggregator code, a row stride below its row, out == a or b -> BOT_E_RANGE; n_rows = 0 -> 0, nothing launched; NULL aggs, items or
 * operands, saved without sarg, S > 1 without scale, long rows without long_rows / long_ptr / workspace -> BOT_E_NULL; a pointer off
 * its 4-byte (items, workspace, partial: 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_pna_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* a, int64_t lda, const float* b,
                     int64_t ldb, int32_t F, int32_t Ft, const int32_t* aggs, int32_t A, const float* scale, int32_t S, int32_t pivot, float* out,
                     int64_t ldo, float* saved, int64_t lds, int32_t* sarg, int64_t ldg, void* workspace, bot_stream_t stream);
int bot_pna_bwd_prep_f32(const int32_t* indptr, int64_t n_rows, const float* dout, int64_t ldd, const float* scale, int32_t S, const int32_t* aggs,
                         int32_t A, int32_t F, int32_t Ft, const float* saved, int64_t lds, const int32_t* sarg, int64_t ldg, float* db, int64_t ldb,
                         float* rec, int64_t ldr, bot_stream_t stream);
int bot_spmm_pna_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                         const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const int32_t* pos, const float* a, int64_t lda,
                         const float* rec, int64_t ldr, const int32_t* aggs, int32_t A, int32_t F, float* dx, int64_t ldx, float* partial,
                         bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PNA aggregation with edge features (csrc/spmm_pna_edge.hip): the PNA aggregation above over per-EDGE messages whose edge term is a
 * projection of K raw edge features formed inside the sweep - DGL's PNAConv(edge_feat_size=K) pretrans M(cat[h_u, h_v, e_uv]), which
 * is linear.  bot_amd.nn.EdgePNAConv, ops.pna_aggregate_edge.  Purely additive to ABI 19.
 *
 * ef float32 [E, K] contiguous, 1 <= K <= 16, read at row eperm[k] of position k (eperm int32 [nnz], rows not range-checked; NULL: row
 * k itself); wt float32 [K, F] contiguous, the projection transposed.  For position k of row r, per column f:
 *   c_k = ef[e,0] wt[0,f], then fmaf(ef[e,j], wt[j,f], c) for j = 1 .. K-1 in index order (a rounded product, then K - 1 fused
 *         multiply-adds; the kernels pad K to 4 / 8 / 16 with zeros, which add +0);  m_k = fl(a[indices[k]] + c_k)
 * and b[r] enters behind the reduce as above (std and var ignore b; they no longer ignore the edge term).  Max and min run on m_k with
 * the strict compares in position order (earliest position of a tie, -0.0 == +0.0, a NaN never enters); sarg holds those positions.
 * Moments use a SPLIT pivot: p_a = a[indices[first]], p_c = c_first of the row's first position, d_k = fl(fl(a_k - p_a) + fl(c_k -
 * p_c)), S1 = sum d_k, S2 = sum d_k^2 in position order; with P = fl(p_a + p_c): mean = fl(P + S1 / n) (+ b), sum = S1 + n P + n b,
 * var, std and the var > 0 gate as above.  A row of constant messages has var = 0 exactly, a shift of a costs nothing, and constant ef
 * across a row gives bot_spmm_pna_f32's S1, S2 bit for bit.  Every chunk of a long row uses the ROW's pivot pair; workspace as above
 * (6 * n_slots * F words).  saved[:, :F] is the mean of the messages without b, saved[:, F:] and sarg as above; an empty row is zeros,
 * positions -1.  Everything else (aggs, scale, Ft, the tower-major layout of out) as in bot_spmm_pna_f32.
 *
 * Backward: bot_pna_bwd_prep_f32 as it is (its "mean of a" section now holds the messages' mean), then bot_spmm_pna_edge_bwd_f32 over
 * the TRANSPOSED direction (rows = sources; pos = Graph.csr2csc, eperm = the ef row of every position of THAT direction): per out-edge
 *   dm_e = g0[v] + c1[v] * fl(fl(a[u] - mu[v]) + c_e) + gmax[v] * (argmax[v] == pos) + gmin[v] * (argmin[v] == pos)
 * with c_e formed again by the same chain;  dx[u] (or NULL) = the sum of dm_e over the out-edges of u in position order (long rows
 * through `partial`, n_slots * F floats);  dweight float32 [F, K] (or NULL) = the sum over ALL edges of ef[e, j] dm_e[f], summed per
 * workgroup in item order, folded through dw_workspace [dw_rows, K, F] (16-byte aligned; dw_rows >= min(1024, n_items / 16 + 1) always
 * suffices) in workgroup order: a grid that depends on (n_items, F) only, never on the device.  Both NULL: 0, nothing launched.  ef gets
 * no gradient.
 *
 * No atomics; the bytes of every output repeat from call to call.
 * Checked before any launch: what bot_spmm_pna_f32 / bot_spmm_pna_bwd_f32 check, and K outside 1 .. 16, a negative dw_rows, a
 * dw_workspace too small for the sweep's grid, out == ef or wt -> BOT_E_RANGE; NULL wt, NULL ef with nnz > 0, dweight without
 * dw_workspace -> BOT_E_NULL; ef, wt, eperm off 4-byte (dw_workspace: 16-byte) alignment -> BOT_E_ALIGN.  n_rows = 0 -> 0 (dweight
 * is zeroed).
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_pna_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                          const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* a, int64_t lda,
                          const float* b, int64_t ldb, int32_t F, int32_t Ft, const float* ef, int32_t K, const int32_t* eperm, const float* wt,
                          const int32_t* aggs, int32_t A, const float* scale, int32_t S, float* out, int64_t ldo, float* saved, int64_t lds,
                          int32_t* sarg, int64_t ldg, void* workspace, bot_stream_t stream);
int bot_spmm_pna_edge_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                              const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const int32_t* pos, const float* a, int64_t lda,
                              const float* ef, int32_t K, const int32_t* eperm, const float* wt, const float* rec, int64_t ldr,
                              const int32_t* aggs, int32_t A, int32_t F, float* dx, int64_t ldx, float* partial, float* dweight,
                              float* dw_workspace, int64_t dw_rows, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Softmax aggregation (csrc/spmm_softmax.hip): the per-channel softmax aggregator of DeeperGCN (Li, Xiong, Thabet, Ghanem,
 * arXiv:2006.07739; GENConv), forward and backward.  Purely additive to ABI 19.
 *
 * For a destination v with in-edges at positions k (sources u_k, parallel edges counted separately) and a column f:
 *   m_k      = relu ? max(x[u_k, f], 0) + eps : x[u_k, f]                      (the message depends on the source only)
 *   a_k      = exp(beta * m_k - lse[v, f]),   lse[v, f] = log sum_k exp(beta * m_k)
 *   out[v,f] = sum_k a_k * m_k;   q[v,f] = sum_k a_k * m_k^2                   (q only when asked for: q != NULL)
 * beta is ONE float32 read from DEVICE memory (a learnable beta costs no host read).  A row without in-edges gives out = lse = q = 0.
 * Non-finite inputs may turn the outputs of their own rows into NaN; they do not reach other rows and nothing faults.  Under relu a
 * NaN entry stays a NaN (the message is a select, not a max that would drop it).
 *
 * Forward, over a direction with its row plan (rows = destinations): x float32 [n_src, F] (row stride ldx >= F, unit inner stride,
 * indices < n_src not checked); out, lse, q float32 [n_rows, F] (ldo, ldl, ldq).  An online softmax per column in position order, one
 * exponential per gathered entry; out = S / Z by a true division (beta = 0: out is float32(sum of m) / float32(degree), bit for bit),
 * lse = M + log Z, q = Q / Z.  Rows longer than the plan's chunk leave their state per chunk in `workspace` ((q ? 4 : 3) * n_slots * F
 * floats, 16-byte aligned; may be NULL without long rows) and are folded in slot order.  Lane layout as in bot_spmm_max_f32.
 *
 * Backward, over the TRANSPOSED direction (rows = sources, indices = destinations): x float32 [n_rows, F] (ldx); dout, out, lse
 * float32 indexed by `indices` (ldd, ldo, ldl); dx float32 [n_rows, F] (lddx).  With m_u as above and gate = relu ? x[u,f] > 0 : 1:
 *   dx[u,f] = gate * sum_j dout[v_j,f] * exp(beta * m_u - lse[v_j,f]) * (1 + beta * (m_u - out[v_j,f]))   over the positions j of row u,
 * in position order; long rows chunk by chunk into `partial` (n_slots * F floats, 16-byte aligned) and added in slot order.  Nothing is
 * stored per edge.  d out / d beta = q - out^2 is a dense reduction over [n_dst, F] and left to the caller.
 *
 * No atomics; the bytes of out, lse, q and dx repeat from call to call.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, F < 1, a non-finite eps, a row stride below F, out / lse / q
 * aliasing x or each other, dx aliasing an input -> BOT_E_RANGE; n_rows = 0 -> 0, nothing launched; NULL items, beta or operands, long
 * rows without long_rows / long_ptr / workspace -> BOT_E_NULL; a pointer off its 4-byte (items, workspace, partial: 16-byte)
 * alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_softmax_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                         const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* x, int64_t ldx, int32_t F,
                         const float* beta, int32_t relu, float eps, float* out, int64_t ldo, float* lse, int64_t ldl, float* q, int64_t ldq,
                         void* workspace, bot_stream_t stream);
int bot_spmm_softmax_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* x, int64_t ldx, const float* beta,
                             int32_t relu, float eps, const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse, int64_t ldl,
                             int32_t F, float* dx, int64_t lddx, float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Softmax aggregation with edge features (csrc/spmm_softmax_edge.hip): the softmax aggregation above over per-EDGE messages whose
 * edge term is projected inside the sweep from K raw edge features (GENConv with edge_dim = K), so no [E, F] operand exists.  Purely
 * additive to ABI 19.
 *
 * Operands beside those of bot_spmm_softmax_f32 / bot_spmm_softmax_bwd_f32: ef float32 [E, K] contiguous, 1 <= K <= 16; eperm int32
 * [nnz], the row of ef of the direction's position k (NULL: k itself; csc.eid / csr.eid for ef in edge-id order); wt float32 [K, F]
 * contiguous, the encoder's weight TRANSPOSED; bias float32 [F] or NULL.  For the edge at position k with source u_k and a column f:
 *   z_k = x[u_k, f] + ((ef[r,0] wt[0,f] + ef[r,1] wt[1,f] + ... + ef[r,K-1] wt[K-1,f]) + bias[f]),   r = eperm ? eperm[k] : k
 * the sum taken in index order as a chain of fused multiply-adds whose first term is a rounded product, then the bias (0 without one),
 * then x: K + 2 roundings, the same float32 in both sweeps.
 *   m_k = relu ? (z_k < 0 ? 0 : z_k) + eps : z_k        (a select: a NaN stays a NaN)
 * Rows of ef are not range-checked (eperm values < E, like indices < n_src).
 *
 * Forward (rows = destinations): out, lse, q as in bot_spmm_softmax_f32 over the m_k of the row's positions, in position order; the
 * long rows' workspace and fold are the same ((q ? 4 : 3) * n_slots * F floats).
 *
 * Backward, over the TRANSPOSED direction (rows = sources u, indices = destinations v_j): with a_j = exp(beta m_j - lse[v_j,f]), c_j =
 * 1 + beta (m_j - out[v_j,f]) and gate_j = relu ? z_j > 0 : 1,
 *   dz_j        = gate_j ? dout[v_j,f] a_j c_j : 0
 *   dx[u,f]     = sum over the positions j of row u of dz_j, in position order           (dx float32 [n_rows, F], lddx; NULL: not computed)
 *   dweight[f,i] = sum over ALL positions of ef[r_j, i] dz_j                             (dweight float32 [F, K] contiguous; NULL: not computed)
 * dx: long rows through `partial` (n_slots * F floats) and the slot-order sum.  dweight: a persistent sweep keeps per-lane sums,
 * folds a workgroup's lane groups in group order and leaves one [K, F] partial per workgroup in dw_workspace (dw_rows * K * F floats,
 * 16-byte aligned); the workgroups are added in index order.  The number of workgroups is a function of n_items, F, K and the
 * operands' alignment only, at most min(1024, n_items / 16 + 1): a dw_workspace of that many rows always suffices, a smaller one that
 * does not is refused.  d bias[f] = sum_u dx[u,f] and d beta = sum dout (q - out^2) are dense reductions left to the caller; ef gets no gradient.
 *
 * No float atomics; the bytes of out, lse, q, dx and dweight repeat from call to call.
 * Checked before any launch: as bot_spmm_softmax_f32 / bot_spmm_softmax_bwd_f32, and K outside 1 .. 16, a dw_workspace too small ->
 * BOT_E_RANGE; NULL wt, NULL ef with nnz > 0, dweight without dw_workspace -> BOT_E_NULL.  Backward: neither dx nor dweight -> 0,
 * nothing launched; n_rows = 0 -> dweight is zeroed.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_softmax_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                              const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* x, int64_t ldx,
                              int32_t F, const float* ef, int32_t K, const int32_t* eperm, const float* wt, const float* bias, const float* beta,
                              int32_t relu, float eps, float* out, int64_t ldo, float* lse, int64_t ldl, float* q, int64_t ldq, void* workspace,
                              bot_stream_t stream);
int bot_spmm_softmax_edge_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                                  int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* x, int64_t ldx,
                                  const float* ef, int32_t K, const int32_t* eperm, const float* wt, const float* bias, const float* beta,
                                  int32_t relu, float eps, const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse,
                                  int64_t ldl, int32_t F, float* dx, int64_t lddx, float* partial, float* dweight, float* dw_workspace,
                                  int64_t dw_rows, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GATv2 edge logits (csrc/gatv2.hip): the attention score of Brody, Alon, Yahav, "How Attentive are Graph Attention Networks?"
 * (ICLR 2022), DGL's GATv2Conv, with its two backward sweeps.  Purely additive to ABI 19.
 *
 * fs float32 [n_src, H*D] (row stride ldfs >= H*D), fd float32 [n_dst, H*D] (ldfd), attn float32 [H*D] (contiguous), unit inner strides;
 * lrelu(s) = s > 0 ? s : slope * s,  lrelu'(s) = s > 0 ? 1 : slope (so lrelu'(0) = slope, torch's convention);  s[k,h,d] =
 * fs[u_k,h,d] + fd[v_k,h,d] for the edge at position k of the direction, u_k its source, v_k its destination.
 *
 * Forward, over the direction whose rows are the destinations (the CSC) with its row plan (indices < n_src not checked):
 *   e[o(k), h] = sum_d attn[h,d] * lrelu(s[k,h,d]),   o(k) = operm ? operm[k] : k,   e float32 [nnz, H] (row stride lde >= H).
 * The sum over d runs in a fixed order per (k, h); one store per (k, h) unless the head spans feature tiles (then one per tile, added in
 * tile order by the same wavefront).
 *
 * Backward over the destinations (the same direction), de float32 [nnz, H] (ldde), read at row dperm ? dperm[k] : k:
 *   t[k,h,d]  = de[k,h] * attn[h,d] * lrelu'(s[k,h,d])
 *   dfd[v]    = sum over the positions k of row v of t[k], in position order (dfd float32 [n_rows, H*D], lddfd; NULL: not computed)
 *   dattn[h,d] = sum over all k of de[k,h] * lrelu(s[k,h,d])                   (dattn float32 [H*D] contiguous; NULL: not computed)
 * Long rows leave one row per chunk in the workspace and are added in slot order; the dattn sums are kept per lane, folded per
 * workgroup in group order into one workspace row per workgroup (at most 2048) and reduced per column in a fixed order.  workspace:
 * bot_gatv2_logits_bwd_dst_workspace_floats(n_items, n_slots, H, D) floats, 16-byte aligned (NULL allowed without long rows and dattn).
 *
 * Backward over the sources, over the TRANSPOSED direction (rows = sources, indices = destinations < n_dst) with pos int32 [nnz]: the
 * row of de of each entry (Graph.csr2csc for de in CSC position order):
 *   dfs[u] = sum over the positions j of row u of t[pos[j]], in position order (dfs float32 [n_rows, H*D], lddfs);
 * long rows through `partial` (n_slots * H*D floats, 16-byte aligned) and the slot-order combine.
 *
 * No float atomics; e, dfd, dattn and dfs repeat their bytes from call to call.  Lane layout as in bot_spmm_max_f32, with vectors of
 * 4 / 2 / 1 floats chosen so that they divide D and the row strides.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, H < 1, D < 1, H*D >= 2^24, a NaN slope, a row stride below its
 * row, dfd / dfs aliasing fs or fd -> BOT_E_RANGE; n_rows = 0 (forward: or nnz = 0; backward over destinations: or neither output
 * asked for) -> 0, nothing launched; NULL items or operands, long rows without long_rows / long_ptr / workspace -> BOT_E_NULL; a
 * pointer off its 4-byte (items, workspace, partial: 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_gatv2_logits_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                         const float* fs, int64_t ldfs, const float* fd, int64_t ldfd, const float* attn, int32_t H, int32_t D, float slope,
                         const int32_t* operm, float* e, int64_t lde, bot_stream_t stream);
int64_t bot_gatv2_logits_bwd_dst_workspace_floats(int64_t n_items, int64_t n_slots, int32_t H, int32_t D);
int bot_gatv2_logits_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                                 const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* fs, int64_t ldfs,
                                 const float* fd, int64_t ldfd, const float* attn, int32_t H, int32_t D, float slope, const float* de, int64_t ldde,
                                 const int32_t* dperm, float* dfd, int64_t lddfd, float* dattn, float* workspace, bot_stream_t stream);
int bot_gatv2_logits_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                                 const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const int32_t* pos, const float* fs, int64_t ldfs,
                                 const float* fd, int64_t ldfd, const float* attn, int32_t H, int32_t D, float slope, const float* de, int64_t ldde,
                                 float* dfs, int64_t lddfs, float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gated aggregation (csrc/spmm_gate.hip): the per-channel sigmoid gate of Bresson & Laurent, "Residual Gated Graph ConvNets"
 * (arXiv:1711.07553) - the GatedGCN of Dwivedi et al., "Benchmarking Graph Neural Networks" (arXiv:2003.00982), PyG's
 * ResGatedGraphConv - forward and its two backward sweeps.  Purely additive to ABI 19.
 *
 * k float32 [n_dst, F] (row stride ldk >= F), q and v float32 [n_src, F] (ldq, ldv), unit inner strides.  q and v are two pointers with
 * a stride each, so they may be the two column blocks of ONE [n_src, 2F] matrix (a neighbour's gate row and value row are then one
 * contiguous gathered row) or two matrices.  For the position j of a direction, with source u and destination w, and a column f:
 *   s    = k[w,f] + q[u,f]
 *   e    = exp(-|s|)                      (the exponential of the softmax sweeps: v_exp_f32 with a first-order correction, <= 4 units of 2^-24)
 *   g    = (s >= 0 ? 1 : e) / (1 + e)     (= sigmoid(s))
 *   gbar = (s >= 0 ? e : 1) / (1 + e)     (= 1 - sigmoid(s), formed directly, never as 1 - g)
 *   g'   = g * gbar
 * Both quotients are true divisions, so g, gbar and g' carry a RELATIVE error bound (8 units of 2^-24 for g and gbar) in both tails, and
 * three regimes are exact bit for bit: s = 0 gives g = gbar = 0.5; s >= 105 gives g = 1, g' = 0; s <= -105 gives g = 0, g' = 0.
 *
 * Forward, over the direction whose rows are the destinations (the CSC) with its row plan (indices < n_src not checked):
 *   num[w,f] = sum_j g_j v[u_j,f],  den[w,f] = sum_j g_j     in position order (num: a chain of fused multiply-adds)
 *   normalize = 0:  out = num; den is neither computed nor stored (pass NULL)
 *   normalize = 1:  out = num / (den + eps) by a true division, den float32 [n_rows, F] (ldden) is stored for the backward
 * A row without in-edges gives out = den = 0.  Rows longer than the plan's chunk leave (num[, den]) per chunk in `workspace`
 * ((normalize ? 2 : 1) * n_slots * F floats, 16-byte aligned; may be NULL without long rows) and are folded in slot order before the
 * division.
 *
 * Backward over the destinations (the same direction).  a float32 [n_rows, F] (lda) and b float32 [n_rows, F] (ldb) or NULL, formed by the
 * caller with dense ops: a = dout / (den + eps), b = -a * out for the normalised form; a = dout, b = NULL otherwise.
 *   ds_j  = g'_j * (v[u_j,f] * a[w,f] + b[w,f])          (the parenthesis one fused multiply-add; without b the rounded product)
 *   dk[w] = sum_j ds_j   in position order (a chain of fused multiply-adds), dk float32 [n_rows, F] (lddk)
 * Long rows through `partial` (n_slots * F floats, 16-byte aligned) and the slot-order sum.
 *
 * Backward over the sources, over the TRANSPOSED direction (rows = sources u, indices = destinations w_j < n_dst): gathers k, a and b of
 * each destination.
 *   dq[u] = sum_j ds_j,   dv[u] = sum_j g_j * a[w_j]     in position order; dq, dv float32 [n_rows, F] (lddq, lddv)
 * Each is computed only when its pointer is not NULL (neither: 0, nothing launched); two pointers with a stride each, so they may be
 * the column blocks of one [n_src, 2F] gradient.  Long rows through `partial` ((dq and dv ? 2 : 1) * n_slots * F floats).
 *
 * Nothing is stored per edge: the gates are formed again in both backward sweeps.  No atomics; out, den, dk, dq and dv repeat their bytes
 * from call to call.  Non-finite inputs may turn the outputs of their own rows into NaN; they do not reach other rows and nothing
 * faults.  Lane layout as in bot_spmm_max_f32.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, F < 1, a non-finite or negative eps, a row stride below F, an
 * output aliasing an input or another output -> BOT_E_RANGE; n_rows = 0 -> 0, nothing launched; NULL items or operands, normalize
 * without den, long rows without long_rows / long_ptr / workspace -> BOT_E_NULL; a pointer off its 4-byte (items, workspace, partial:
 * 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_gate_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                      const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* k, int64_t ldk,
                      const float* q, int64_t ldq, const float* v, int64_t ldv, int32_t F, int32_t normalize, float eps, float* out, int64_t ldo,
                      float* den, int64_t ldden, void* workspace, bot_stream_t stream);
int bot_spmm_gate_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                              int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* k, int64_t ldk,
                              const float* q, int64_t ldq, const float* v, int64_t ldv, const float* a, int64_t lda, const float* b, int64_t ldb,
                              int32_t F, float* dk, int64_t lddk, float* partial, bot_stream_t stream);
int bot_spmm_gate_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                              int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* k,
                              int64_t ldk, const float* q, int64_t ldq, const float* v, int64_t ldv, const float* a, int64_t lda, const float* b,
                              int64_t ldb, int32_t F, float* dq, int64_t lddq, float* dv, int64_t lddv, float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gated aggregation with an edge stream (csrc/spmm_gate_edge.hip): GatedGCN as "Benchmarking Graph Neural Networks" (arXiv:2003.00982)
 * and GraphGPS run it, DGL's GatedGCNConv - the gate of the section above with a per-EDGE term in its pre-activation, which is also the
 * layer's second output.  Purely additive to ABI 19.
 *
 * k float32 [n_dst, F] (ldk), q and v float32 [n_src, F] (ldq, ldv; two pointers with a stride each, so they may be the two column blocks
 * of ONE [n_src, 2F] matrix), unit inner strides.  The per-edge operands c, e, de and ds are float32 [nnz, F] in the POSITION order of
 * the direction whose rows are the destinations (the CSC), unit inner stride, a row pitch each (ldc, lde, ldde, ldds >= F).  The gate
 * (g, gbar, g' = g gbar) is the one of "Gated aggregation", with its error bounds and its three exact regimes.
 *
 * Forward, over the CSC with its row plan (indices < n_src not checked).  For the position j of row w with source u and a column f:
 *   s_j  = (k[w,f] + q[u,f]) + c[j,f]        two rounded additions, in that order
 *   e[j,f] = s_j                             stored unless e is NULL
 *   num[w,f] = sum_j g(s_j) v[u,f],  den[w,f] = sum_j g(s_j)      in position order (num: a chain of fused multiply-adds)
 *   normalize = 0:  out = num; den is neither computed nor stored (pass NULL)
 *   normalize = 1:  out = num / (den + eps) by a true division, den float32 [n_rows, F] (ldden) is stored for the backward
 * A row without in-edges gives out = den = 0 and touches no row of e.  k[w] stays in registers across the row; c[j] and e[j] are
 * streamed at the walk's position.  e MAY ALIAS c (the same pointer and pitch): every element is read and then written by the same
 * lane.  Rows longer than the plan's chunk: every chunk stores e for its own positions and leaves (num[, den]) in `workspace`
 * ((normalize ? 2 : 1) * n_slots * F floats, 16-byte aligned; may be NULL without long rows), folded in slot order before the division.
 * HBM model: 4 [nnz (1 + 2F + 2F) + n_rows F (2 or 3)] bytes.
 *
 * Backward over the CSC (the same direction).  e: the forward's stored float32 rows (k, q and c are not read again); a float32
 * [n_rows, F] (lda) and b float32 [n_rows, F] (ldb) or NULL, formed by the caller: a = dout / (den + eps), b = -a * out for the normalised
 * form; a = dout, b = NULL otherwise.  de float32 [nnz, F] (ldde): the upstream gradient of e, NULL counts as zero.
 *   ds[j,f] = de[j,f] + g'(e[j,f]) * (v[u,f] * a[w,f] + b[w,f])     the parenthesis one fused multiply-add (without b the rounded product),
 *                                                                  then the rounded product with g', then the rounded addition of de
 *   dk[w,f] = sum_j ds[j,f]   in position order, dk float32 [n_rows, F] (lddk)
 * ds is the gradient of c and the operand of the source side.  ds MAY ALIAS de (the same pointer and pitch).  Either of ds and dk may be
 * NULL and is then not computed (both: 0, nothing launched).  Long rows: every chunk stores ds for its own positions; dk through
 * `partial` (n_slots * F floats, 16-byte aligned; not needed without dk) and the slot-order sum.
 * HBM model: 4 [nnz (1 + 4F) + n_rows F (2 or 3)] bytes, less 4 nnz F where de is NULL.
 *
 * Backward over the sources, over the TRANSPOSED direction (rows = sources u, indices = destinations w_j < n_dst) with pos int32 [nnz], the
 * CSC position of every entry (Graph.csr2csc; pos < nnz not checked):
 *   dq[u,f] = sum_j ds[pos_j,f],   dv[u,f] = sum_j g(e[pos_j,f]) * a[w_j,f]     in position order; dq, dv float32 [n_rows, F] (lddq, lddv)
 * Each is computed only when its pointer is not NULL (neither: 0, nothing launched), and the rows only the other needs (ds for dq; e and a
 * for dv) are then neither gathered nor required.  Long rows through `partial` ((dq and dv ? 2 : 1) * n_slots * F floats).
 * HBM model: 4 [nnz (2 + 3F) + 3 n_rows F] bytes (a counted once per row).
 *
 * stream_nt != 0 marks the accesses to the streamed rows (c, e, de, ds of the two CSC sweeps) non-temporal; values and bytes do not
 * change.  No atomics; every output repeats its bytes from call to call.  Non-finite inputs may turn the outputs of their own rows
 * into NaN; they do not reach other rows and nothing faults.  Lane layout as in bot_spmm_max_f32.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, F < 1, a non-finite or negative eps, a row stride below F, an
 * output aliasing an input or another output other than as allowed above -> BOT_E_RANGE; n_rows = 0 -> 0, nothing launched; NULL items
 * or operands, normalize without den, long rows without long_rows / long_ptr / workspace -> BOT_E_NULL; a pointer off its 4-byte (items,
 * workspace, partial: 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_gate_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                           const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* k, int64_t ldk,
                           const float* q, int64_t ldq, const float* v, int64_t ldv, const float* c, int64_t ldc, int32_t F, int32_t normalize,
                           float eps, float* out, int64_t ldo, float* den, int64_t ldden, float* e, int64_t lde, int32_t stream_nt,
                           void* workspace, bot_stream_t stream);
int bot_spmm_gate_edge_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                               int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* v, int64_t ldv,
                               const float* e, int64_t lde, const float* a, int64_t lda, const float* b, int64_t ldb, const float* de,
                               int64_t ldde, int32_t F, float* ds, int64_t ldds, float* dk, int64_t lddk, int32_t stream_nt, float* partial,
                               bot_stream_t stream);
int bot_spmm_gate_edge_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                                   int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots,
                                   const int32_t* pos, const float* e, int64_t lde, const float* ds, int64_t ldds, const float* a, int64_t lda,
                                   int32_t F, float* dq, int64_t lddq, float* dv, int64_t lddv, float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Relational aggregation (csrc/spmm_rel.hip): the two sweeps of the relational GCN (Schlichtkrull et al., "Modeling Relational Data with
 * Graph Convolutional Networks", ESWC 2018; DGL's RelGraphConv, PyG's RGCNConv) with the basis regulariser W_r = sum_b coef[r,b] V_b.
 * Purely additive to ABI 19.
 *
 * Over one direction with its row plan (indices < n_src not checked).  Per position j of row v: the neighbour u_j = indices[j], the
 * relation r_j = etype[j] (int32 [nnz] in this direction's POSITION order; 0 <= r_j < R is NOT checked per launch: the caller checks it
 * once) and the constant weight c_j = norm[j] (float32 [nnz] in position order; NULL: c_j = 1.0f, the bytes of a norm of ones).
 * coef float32 [R, B] contiguous, or NULL for the one-hot mode: B = R and coef the identity (pass B = R or 0), never stored.
 *   expand    Z[v,b,:]  = sum_j c_j coef[r_j,b] x[u_j,:]          x float32 [n_src, F] (row stride ldx >= F) -> out float32 [n_rows, B, F]
 *                                                                  (row stride ldo >= B F, block b at column b F); one-hot: the row is
 *                                                                  added into block r_j alone
 *   contract  out[v,:]  = sum_j c_j sum_b coef[r_j,b] y[u_j,b,:]  y float32 [n_src, B, F] (ldy >= B F) -> out float32 [n_rows, F] (ldo >= F);
 *                                                                  one-hot: block r_j of the row alone is gathered (F floats per edge)
 * Unit inner strides.  The two are each other's transpose: the gradient of one over a direction is the other over the transposed
 * direction with the same etype, norm and coef (in that direction's position order).
 * Sums run in position order in registers: expand w = c_j * coef[r_j,b], acc_b = fma(w, x, acc_b); contract t = sum over b in order (a
 * product, then fused multiply-adds), acc = fma(c_j, t, acc).  At most 16 blocks per pass: expand walks a row ceil(B / 16) times (each
 * pass gathers again), contract likewise on one accumulator (pass-major order); the one-hot contract is one pass whatever R is.  A row
 * without entries gives zeros.  Rows longer than the plan's chunk leave their sums per chunk in `workspace` (n_slots * B * F floats for
 * expand, n_slots * F for contract, 16-byte aligned; may be NULL without long rows) and are folded in slot order.  No atomics: two
 * calls give the same bytes.  Non-finite inputs stay in their own rows.
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, F < 1, R < 1, B < 1 with coef (B not R or 0 without), B * F >= 2^31,
 * a row stride below the row, out aliasing the input, long rows without slots -> BOT_E_RANGE; n_rows = 0 -> 0, nothing launched; NULL
 * items or out, with nnz > 0 NULL indices / etype / input, long rows without long_rows / long_ptr / workspace -> BOT_E_NULL; a pointer off
 * its 4-byte (items, workspace: 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_spmm_rel_expand_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                            const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const int32_t* etype,
                            const float* norm, const float* coef, int32_t R, int32_t B, const float* x, int64_t ldx, int32_t F, float* out,
                            int64_t ldo, void* workspace, bot_stream_t stream);
int bot_spmm_rel_contract_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                              const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const int32_t* etype,
                              const float* norm, const float* coef, int32_t R, int32_t B, const float* y, int64_t ldy, int32_t F, float* out,
                              int64_t ldo, void* workspace, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dot-product attention (csrc/dot_attn.hip): scaled dot-product attention over a node's in-edges - the layer of UniMP (Shi et al.,
 * arXiv:2009.03509), PyG's TransformerConv, DGL's DotGatConv - as one fused online-softmax sweep with its two backward sweeps.
 * Purely additive to ABI 19.
 *
 * q float32 [n_dst, H*D] (row stride ldq >= H*D), k / v float32 [n_src, H*D] (ldk, ldv), unit inner strides.  Per head h, with u_k the
 * source of the edge at position k of row v:  s_k = scale * sum_d q[v,h,d] k[u_k,h,d];  keep int32 [nnz] in position order, bit h =
 * head h of that edge is kept (NULL: every edge is kept and c = 1), else c = 1 / (1 - p).
 *
 * Forward, over the direction whose rows are the destinations (the CSC) with its row plan (indices < n_src not checked):
 *   lse[v,h] = log sum_k exp(s_k),  a_k = exp(s_k - lse[v,h]),  out[v,h,:] = c sum_k keep_k,h a_k v[u_k,h,:];  an empty row: out = lse = 0.
 *   out float32 [n_rows, H*D] (ldo), lse float32 [n_rows, H] (ldl >= H).  An online softmax in position order (the normaliser counts
 *   every edge, the sum only the kept ones), out = c * (S / Z) by a true division.  k == v with ldk == ldv: one gather per edge.
 *   Long rows leave their chunks' states in `workspace` (n_slots * (H*D + 2 H) floats, 16-byte aligned) and are folded in slot order.
 * Backward over the destinations (the same direction), dout [n_rows, H*D] (ldd), out and lse as the forward left them:
 *   delta[v,h] = sum_d dout[v,h,d] out[v,h,d],  dd_k = sum_d dout[v,h,d] v[u_k,h,d],  p[k,h] = c keep_k,h a_k,
 *   ds[k,h] = a_k (c keep_k,h dd_k - delta[v,h]),  dq[v,h,:] = scale sum_k ds[k,h] k[u_k,h,:]   (dq [n_rows, H*D], lddq; NULL: not computed)
 *   p and ds: float32 [nnz, H] contiguous, position order, always written.  Long rows through `partial` (n_slots * H*D floats).
 * Backward over the sources, over the TRANSPOSED direction (rows = sources, indices = destinations) with pos int32 [nnz], the row of
 * p / ds of each entry (Graph.csr2csc):
 *   dk[u,h,:] = scale sum_j ds[pos_j,h] q[v_j,h,:],  dv[u,h,:] = sum_j p[pos_j,h] dout[v_j,h,:]   ([n_rows, H*D]; either may be NULL;
 *   dk == dv: one output that holds dk + dv).  Long rows through `partial` (2 * n_slots * H*D floats) and the slot-order combine.
 *
 * No float atomics; every output repeats its bytes from call to call.  Vectors of 4 / 2 / 1 floats chosen so that they divide D and
 * the row strides; a head must fit one tile of 64 * 6 lanes: D / vec > 384 -> BOT_E_RANGE (callers run the tensor form).
 * Checked before any launch: negative sizes, n_rows or nnz >= 2^31, H < 1, D < 1, H*D >= 2^24, a NaN scale, p outside [0, 1), a keep
 * mask with H > 32, a row stride below its row, an output aliasing an input -> BOT_E_RANGE; n_rows = 0 (sources: or neither output
 * asked for) -> 0, nothing launched; NULL items or operands, long rows without long_rows / long_ptr / workspace -> BOT_E_NULL; a
 * pointer off its 4-byte (items, workspace, partial: 16-byte) alignment -> BOT_E_ALIGN.
 * ------------------------------------------------------------------------------------------- */
int bot_dot_attn_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* q, int64_t ldq,
                     const float* k, int64_t ldk, const float* v, int64_t ldv, int32_t H, int32_t D, float scale, const int32_t* keep, float p,
                     float* out, int64_t ldo, float* lse, int64_t ldl, void* workspace, bot_stream_t stream);
int bot_dot_attn_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* q, int64_t ldq, const float* k,
                             int64_t ldk, const float* v, int64_t ldv, int32_t H, int32_t D, float scale, const int32_t* keep, float p,
                             const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse, int64_t ldl, float* pw, float* ds,
                             float* dq, int64_t lddq, float* partial, bot_stream_t stream);
int bot_dot_attn_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const int32_t* pos,
                             const float* q, int64_t ldq, const float* dout, int64_t ldd, const float* pw, const float* ds, int32_t H, int32_t D,
                             float scale, float* dk, int64_t lddk, float* dv, int64_t lddv, float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dot-product attention with edge features (csrc/dot_attn.hip, the EDGE instances): PyG's TransformerConv(edge_dim=K), the layer of UniMP on graphs
 * with edge features.  Purely additive to ABI 19.
 *
 * PyG's layer adds E_e = W ef_e (W = lin_edge.weight viewed [H, D, K], no bias) to the key and to the value of the in-edge e.  Both
 * uses are linear, so the encoder stays outside the sweeps, which see K raw floats per edge:
 *   qe float32 [n_dst, H*K] (ldqe >= H*K): qe[v,h,:] = q[v,h,:] W[h], formed by the caller;  <q[v,h], E_e[h]> = <qe[v,h], ef_e>
 *   ef float32 [nnz, K] (ldef >= K) in POSITION order (row k = the edge at position k of the direction)
 *   aef float32 [n_dst, H*K] (ldae): aef[v,h,:] = c sum_k keep_k,h a_k ef_k;  the caller adds W[h] aef[v,h,:] to out[v,h,:]
 * The other operands, the keep mask and c as in bot_dot_attn_f32 (k and v are always gathered separately: no shared form).
 *
 * Forward:  s_k = scale (sum_d q[v,h,d] k[u_k,h,d] + sum_j qe[v,h,j] ef[k,j]);  lse, a_k, out as bot_dot_attn_f32 with this s_k;  aef as
 *   above, through the same online merge and the same true division;  an empty row: out = lse = aef = 0.  The owner of edge column j is
 *   the j-th vector slot of its head; its product joins the lane's partial logit in front of the head reduction.  workspace:
 *   n_slots * (H*D + 2 H + H*K) floats, 16-byte aligned.
 * Backward over the destinations, dout [n_rows, H*D] (ldd) and daef [n_rows, H*K] (lddae), out / lse / aef as the forward left them:
 *   delta[v,h] = sum_d dout[v,h,d] out[v,h,d] + sum_j daef[v,h,j] aef[v,h,j],  dd_k = sum_d dout[v,h,d] v[u_k,h,d] + sum_j daef[v,h,j] ef[k,j],
 *   p[k,h] = c keep_k,h a_k,  ds[k,h] = a_k (c keep_k,h dd_k - delta[v,h]),  dq[v,h,:] = scale sum_k ds[k,h] k[u_k,h,:]  (lddq; NULL: not
 *   computed),  dqe[v,h,:] = scale sum_k ds[k,h] ef[k,:]  ([n_rows, H*K], lddqe; NULL: not computed).  p and ds as in
 *   bot_dot_attn_bwd_dst_f32: bot_dot_attn_bwd_src_f32 turns them into dk and dv unchanged.  partial: n_slots * (H*D + H*K) floats.
 *   The logit is the forward's float32, product for product.
 *
 * No float atomics; every output repeats its bytes.  Vectors of 4 / 2 / 1 floats as in bot_dot_attn_f32, narrowed until D / vec >= K.
 * Checked before any launch, beside what bot_dot_attn_f32 checks: K < 1, K > 16, D < K -> BOT_E_RANGE (callers run the tensor form).
 * ------------------------------------------------------------------------------------------- */
int bot_dot_attn_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                          const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* q, int64_t ldq,
                          const float* k, int64_t ldk, const float* v, int64_t ldv, const float* qe, int64_t ldqe, const float* ef, int64_t ldef,
                          int32_t H, int32_t D, int32_t K, float scale, const int32_t* keep, float p, float* out, int64_t ldo, float* lse,
                          int64_t ldl, float* aef, int64_t ldae, void* workspace, bot_stream_t stream);
int bot_dot_attn_edge_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                                  int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots,
                                  const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* qe,
                                  int64_t ldqe, const float* ef, int64_t ldef, int32_t H, int32_t D, int32_t K, float scale, const int32_t* keep,
                                  float p, const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse, int64_t ldl,
                                  const float* aef, int64_t ldae, const float* daef, int64_t lddae, float* pw, float* ds, float* dq, int64_t lddq,
                                  float* dqe, int64_t lddqe, float* partial, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Edge-weighted neighbour sampling without replacement (DGL's sample_neighbors(..., prob=w), csrc/sampling_weighted.hip).
 * Purely additive to ABI 19.  Weights w: float32, one per parent edge, in edge-id order.  For seed v with CSC row
 * [base, base + deg) and fan-out k:
 *  1. Quantisation, per row.  w_max = m * 2^e (m in [0.5, 1)) is the row's largest weight; q_i = floor(w[eid[base + i]] * 2^(33 - e)),
 *     exact (a power-of-two scale, then a truncation), so q_max is in [2^32, 2^33) and the row total Q < 2^64 for any int32 row.
 *     A weight below about 2^-33 of its row's largest counts as zero; scaling a row by 2^s leaves the picks unchanged while every
 *     weight stays a normal fp32.
 *  2. Successive sampling: round m (0 <= m < k) draws t = floor(r * Q_rem / 2^96), r = x0 * 2^64 + x1 * 2^32 + x2 from words x0..x2
 *     of Philox4x32-10 under key `seed` at counter v << 32 | m, Q_rem = the total q of the untaken edges, computed exactly as
 *     (hi64 * Q_rem + floor(x2 * Q_rem / 2^32)) >> 64 with hi64 = x0 * 2^32 + x1 (bias below 2^-32).  The round takes the smallest
 *     offset i for which the sum of q_j over untaken j <= i exceeds t (always an untaken edge with q_i > 0).
 *     The same distribution as DGL's weighted pick without replacement: draw in proportion to weight, remove, repeat.
 *  3. A row with at most k edges of positive q gives all of them (k < 0: always); an edge with q = 0 is never taken.
 *  4. Output as bot_sample_neighbors_i32: parent CSC positions, ascending per seed, into out[offsets[i] .. offsets[i+1]).
 *  5. A pure function of (graph, weights, seeds, k, seed): independent of where v sits in the seed list and of the launch shape.
 *
 * prepare:  once per weight tensor.  prefix uint64 [n_edges] in CSC position order = the inclusive scan of q within each row;
 *           n_pos int32 [n_rows] = edges of positive q per row; flag: one int32 of device scratch.  8 B per edge (about 1 GB at
 *           S-products, 0.6 GB at S-proteins).  A negative, NaN or infinite weight -> BOT_E_RANGE, found with one device->host read
 *           (the call synchronises the stream).
 * count:    counts[i] = min(k, n_pos[seeds[i]]), n_pos[seeds[i]] for k < 0.
 * sample:   one wavefront per seed; k serial rounds of a 64-ary search of the prefix corrected by the taken set (sorted in LDS),
 *           O(k (log_64 deg + k / 64)) per row.  LDS 12 * k B per wave.  No float arithmetic, no atomics: deterministic.
 * Argument checks: NULL pointers -> BOT_E_NULL, negative sizes / k > 1024 -> BOT_E_RANGE, no seeds (no rows) -> 0 (nothing launched).
 * ------------------------------------------------------------------------------------------- */
int bot_sample_weights_prepare_f32(const int32_t* indptr, const int32_t* eid, int64_t n_rows, int64_t n_edges, const float* w,
                                   uint64_t* prefix, int32_t* n_pos, int32_t* flag, bot_stream_t stream);
int bot_sample_neighbors_weighted_count_i32(const int32_t* n_pos, int64_t n_rows, const int32_t* seeds, int64_t n_seeds, int32_t k,
                                            int32_t* counts, bot_stream_t stream);
int bot_sample_neighbors_weighted_i32(const int32_t* indptr, const uint64_t* prefix, const int32_t* n_pos, int64_t n_rows, const int32_t* seeds,
                                      int64_t n_seeds, int32_t k, uint64_t seed, const int64_t* offsets, int32_t* out, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * fp32 GEMMs on the fp16 matrix cores.  The dense projections of the layer (`self.fc`, `self.res_fc`, the folded attention
 * columns: src/no-sampling/models.py:490-492, :519-522, :553-557; their backward) are fp32 GEMMs of [N, 750] x [750, 1536]
 * size, MFMA-bound at gfx950's fp32 rate.  Each fp32 operand is written as two fp16 halves, x = (h1 + h2) / s with
 * h1 = fp16(fp32(s x)), h2 = fp16(fma(x, s, -h1)) - s x - h1 in ONE rounding: for a power-of-two s it is exact, and where s x leaves
 * float32's range it is an infinity resp. a signed zero, not inf - inf = NaN -, s a power of two chosen ON THE DEVICE from max|x| (halves_scale: scale[0] = s,
 * scale[1] = 1/s), and a product is evaluated as a1 b1 + a1 b2 + a2 b1 with fp32 accumulation: ONE fp16 GEMM over the
 * concatenated reduction axis.  h1 + h2 carries 22-23 of the 24 significand bits; against fp64 the result is as close as
 * hipBLASLt's fp32 GEMM (tools/exp_split_gemm*.py), at ~3x its speed.
 *
 *   halves_split  out[r, :] = [h1 | h1 | 2^11 h2] (order 0: left operands) or [h1 | h2 | 2^-11 h1] (order 1: right operands) or, v15,
 *                 [h1 | 2^11 h2] (order 2: a left operand WITHOUT the duplicate h1 piece, row pitch >= 2 * piece — only the library's
 *                 concatenated-axis GEMM reads the duplicate; bot_gemm_halves3_nt_f32 / _tn_f32 take the offset of the second half), every
 *                 piece `piece` >= F columns wide (zero padded; use a multiple of 64), out fp16 with row pitch ldo >= 3 * piece
 *                 (order 2: >= 2 * piece).
 *                 The 2^11 keeps a left operand's second half in fp16's normal range: ROWS down to 2^-28 of the matrix maximum keep
 *                 22 significant bits (one scale per matrix alone: 2^-17), and every entry is reproduced to 2^-38 of the matrix
 *                 maximum in absolute terms.  A product of two LEFT layouts (x^T d, the weight gradient) is formed from separate
 *                 GEMMs over the pieces with the 2^-11 applied by the caller (bot_amd/gemm.py:tn).
 *   gemm_halves   C[m,n] = alpha[j] * op(A)[m,k] op(B)[k,n] + beta * C[m,n], row-major, A / B fp16, C fp32, `alpha` a DEVICE vector of n
 *                 floats (one per output column; normally n copies of the product of the two operands' 1/s); trans_x != 0: the operand is stored transposed.  batch > 1: strided
 *                 batches (element strides).  Kernel choice: `algo_index` >= 0 = a solution index recorded for this shape on this library
 *                 build (bot_amd/tuning/halves_gemm.json); else with tune = 0 (what bot_amd passes by default) hipBLASLt's first heuristic
 *                 choice — no timing, no synchronisation, the same kernel every run.  EXCEPTION to the conventions at the top of this
 *                 header, opt-in only: tune = 1 / 2 makes the FIRST call per shape time the 16 heuristic candidates / all solutions on the
 *                 caller's buffers (beta == 0 only: C is overwritten; never under stream capture) — that call creates events,
 *                 synchronises, and the winner may differ from run to run (different accumulation order).  `workspace`: device
 *                 scratch for hipBLASLt (32 MiB is plenty).
 *   bot_gemm_halves_library_version: the hipBLASLt the library was COMPILED against (headers) and the one it is RUNNING on (the
 *                 first libhipblaslt.so.N the process loaded — with PyTorch in the process, the copy torch ships), both as
 *                 major * 100000 + minor * 100 + patch; runtime is 0 before the first gemm_halves call on the current device.
 * ------------------------------------------------------------------------------------------- */
int64_t bot_halves_workspace_floats(void);
int bot_halves_scale_f32(const float* x, int64_t ldx, int64_t n, int32_t F, float* scale, float* workspace, bot_stream_t stream);
/* Maxima as by-products (v12).  The scale of an operand only needs max|x|; when x is a gradient buffer that several kernels have just
 * written, they can deliver it: bot_spmm_dot_f32, bot_bn_act_bwd_apply_f32 and bot_gat_infer_f32 take `absmax_slots`, an array of bot_absmax_slots()
 * uint32 words that the CALLER ZEROES; every workgroup folds the largest |value| it stored into one of them as a bit pattern
 * (non-negative floats order like unsigned integers: an integer atomic max — exact, independent of the order of arrival; NaNs are
 * skipped as in halves_scale).  bot_absmax_slots_f32 adds a strided matrix the slow way (the few columns no producer covers);
 * bot_halves_scale_from_slots_f32 turns the slots into the same (s, 1/s) pair bot_halves_scale_f32 would have found. */
int32_t bot_absmax_slots(void);
int bot_absmax_slots_f32(const float* x, int64_t ldx, int64_t n, int32_t F, uint32_t* slots, bot_stream_t stream);
int bot_halves_scale_from_slots_f32(const uint32_t* slots, float* scale, bot_stream_t stream);
int bot_halves_split_f16(const float* x, int64_t ldx, int64_t n, int32_t F, const float* scale, int32_t order, uint16_t* out,
                         int64_t ldo, int32_t piece, bot_stream_t stream);
/* The same split into a COLUMN RANGE of a wider halves operand: `out` points at the range's first column of piece 0, `width` (even,
 * F <= width <= piece) columns of each of the three pieces are written — F from x, zeros behind them — the pieces stay `piece` apart.
 * Lets several matrices that are one operand side by side (the gradients of a merged projection's column blocks) be split in place,
 * under ONE scale, without first copying them into one buffer. */
int bot_halves_split_cols_f16(const float* x, int64_t ldx, int64_t n, int32_t F, const float* scale, int32_t order, uint16_t* out,
                              int64_t ldo, int32_t piece, int32_t width, bot_stream_t stream);
/* v16: x [n, H * D] as a LEFT operand without the duplicate piece whose head blocks are DP >= D columns wide: out[r, h DP + j] = h1,
 * out[r, h2_off + h DP + j] = 2^11 h2 of scale[0] * x[r, h D + j], zeros for D <= j < DP — H calls of bot_halves_split_cols_f16(order 2) on
 * column slices in one pass (the gradient operand of the aggregate-first GAT layer: every head's block starts on a 128-byte boundary). */
int bot_halves_split_heads_f16(const float* x, int64_t ldx, int64_t n, int32_t H, int32_t D, const float* scale, uint16_t* out, int64_t ldo,
                               int32_t h2_off, int32_t DP, bot_stream_t stream);
/* The weight gradient x^T d of two LEFT-layout operands, formed by the caller from row chunks (batched gemm_halves calls): a [chunks][K][2 PP]
 * = x1^T [d1 | 2^11 d2] and b [chunks][K][PP] = (2^11 x2)^T d1 per chunk, contiguous, plus optional remainder chunks rem_a [K][2 PP] / rem_b [K][PP]:
 *   out[k, p] = sum_c a[c][k][p] + (sum_c a[c][k][PP + p] + sum_c b[c][k][p]) * 2^-11      (chunk order, p < P <= PP)
 * one launch instead of two library reductions and four element-wise passes. */
int bot_halves_tn_combine_f32(const float* a, const float* b, int32_t chunks, int32_t K, int32_t PP, int32_t P, const float* rem_a,
                              const float* rem_b, float* out, int64_t ldo, bot_stream_t stream);
int bot_gemm_halves_f32(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k, const float* alpha, const uint16_t* A,
                        int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc, int32_t batch, int64_t stride_a,
                        int64_t stride_b, int64_t stride_c, float beta, void* workspace, int64_t workspace_bytes, int32_t tune,
                        int32_t algo_index, bot_stream_t stream);
/* v14: the NT product of two halves operands, hand-written for gfx950 (csrc/halves3.hip) instead of the library call above:
 *   C[m, n] = scale_a[1] scale_b[1] * sum_k ( a1[m,k] b1[n,k] + a1[m,k] b2[n,k] + (2^11 a2)[m,k] (2^-11 b1)[n,k] )
 * scale_a / scale_b: the operands' (s, 1/s) device pairs from halves_scale (read by the kernel: no alpha vector, no launch to form it);
 * mode 0 (anything else is an ablation switch of the measurement tools).
 * A: a LEFT operand's buffer (row pitch lda halves; a1 at column 0, 2^11 a2 at column a2_off = 2 * piece), B: a RIGHT operand's buffer
 * (b1 at column 0, b2 at column b2_off = piece); k = the piece width (a multiple of 32).  Each operand half is staged through LDS once
 * per k-step and serves all three MFMAs (the library formulation concatenates the reduction axis three-fold and stages a1 and b1 twice).
 * Same operands, same three products, fp32 accumulation: results differ from bot_gemm_halves_f32 only in summation order.
 * Replaces the projections x W^T of src/no-sampling/models.py:490-492, :558-560 (forward) and their input gradients d W. */
int bot_gemm_halves3_nt_f32(int64_t m, int64_t n, int64_t k, const float* scale_a, const float* scale_b, const uint16_t* A, int64_t lda,
                            int64_t a2_off, const uint16_t* B, int64_t ldb, int64_t b2_off, float* C, int64_t ldc, int32_t mode,
                            bot_stream_t stream);
/* v14: the weight gradient  out[k, p] = scale_x[1] scale_d[1] * sum_n (x1 + x2)[n, k] (d1 + d2)[n, p]  (without the x2 d2 term) of two LEFT
 * operand buffers X [n_rows, ldx] (x1 at column 0, 2^11 x2 at column x2_off = 2 * piece) and D [n_rows, ldd], hand-written for gfx950
 * (csrc/halves3.hip: the reduction index runs along the ROWS of both operands; fragments by the transposing LDS read ds_read_b64_tr_b16;
 * 192 x 192 tiles, three LDS stages, split-K over row ranges with one split per XCD, partials added in split order).  kp / pp: the piece widths (multiples of 64, zero padded beyond k / p);
 * workspace: bot_gemm_halves3_tn_workspace_floats(n_rows, kp, pp) floats; mode 0 (other values: ablation switches of the measurement tools).  Replaces the batched library products + bot_halves_tn_combine_f32
 * for the weight gradients of `fc` / `res_fc` (backward of src/no-sampling/models.py:490-492, 558-560). */
int64_t bot_gemm_halves3_tn_workspace_floats(int64_t n_rows, int64_t kp, int64_t pp);
int bot_gemm_halves3_tn_f32(int64_t n_rows, int64_t k, int64_t p, int64_t kp, int64_t pp, const float* scale_x, const float* scale_d,
                            const uint16_t* X, int64_t ldx, int64_t x2_off, const uint16_t* D, int64_t ldd, int64_t d2_off, float* out,
                            int64_t ldo, float* workspace, int32_t mode, bot_stream_t stream);

/* v17: a hidden layer's gradient operand without a split pass (bot_amd/nn/fused.py:_GATHidden.backward; the backward of
 * src/no-sampling/models.py:490-492, :547, :558-560, :726-731).  The [N, P] gradient of the merged projection's output, [d ft | d res | d el | d er | 0],
 * used to be assembled in fp32 and split into halves by one more pass (1 GB read + 1 GB written at config 2).  Its two big column blocks
 * now leave their producers as halves - d res: bot_bn_act_bwd_apply_halves_f32 (fp32 dx beside it: the sweep gathers those rows), d ft:
 * bot_spmm_dot_halves_f16 - under a scale that must exist BEFORE they run, i.e. a BOUND:
 *     |d res| <= bound of bot_bn_bwd_bound_f32,    |d ft[u,h,:]| <= (sum of the edge weights out of u) max|d res| <= rowsum_bound * max|d res|
 * (bot_halves_scale_from_slots2_f32: the scale of `mult` x the slots' maximum; the format keeps 22 bits for entries down to 2^-28 of the
 * scale, a loose bound costs range, not accuracy).  The handful of attention columns, known only after the sweep and of another magnitude,
 * get a SECOND scale (bot_halves_tail_f16 writes them and the zero padding): the NT product multiplies its accumulators by the ratio of the
 * two scales (powers of two: exact) in front of the k-step where the second range starts, the TN product applies it per output column.
 *   bot_halves_scale_from_slots2_f32   scale = halves_scale(mult * max(slots)); cap_scale != NULL: at most cap_scale[0] * cap_ratio
 *   bot_halves_tail_f16                segments g < n_seg <= 8 of (col, width) = seg_cols[2 g], seg_cols[2 g + 1]: out[r, col + j] = h1,
 *                                      out[r, h2_off + col + j] = 2^11 h2 of scale[0] * srcs[g][r * src_ld[g] + j]  (srcs[g] == NULL: zeros)
 *   bot_spmm_dot_halves_f16            bot_spmm_dot_f32 with `out` replaced by the operand: hout[r, h * hsh + e] (h1) and + h2_off (2^11 h2) of
 *                                      hscale[0] * out[r,h,e]; all-heads layout only (bot_spmm_dot_halves_fits: 1 when the shape and the
 *                                      alignments are covered, else the caller keeps the fp32 form + a split pass)
 *   bot_gemm_halves3_nt2_f32 / _tn2_f32  the products above with the second scale: A's columns >= k_split (a multiple of 32) resp. D's
 *                                      columns >= p_split (a multiple of 4) are stored under scale_a2 / scale_d2 (NULL: one scale). */
int bot_halves_scale_from_slots2_f32(const uint32_t* slots, float mult, const float* cap_scale, float cap_ratio, float* scale, bot_stream_t stream);
int bot_halves_tail_f16(int64_t n, int32_t n_seg, const int64_t* seg_cols, const float* const* srcs, const int64_t* src_ld, const float* scale, uint16_t* out,
                        int64_t ldo, int32_t h2_off, bot_stream_t stream);
int bot_spmm_dot_halves_fits(const float* x, int64_t ldx, int64_t hsx, const float* y, int64_t ldy, int64_t hsy, int32_t H, int32_t D, const uint16_t* hout,
                             int64_t ldh, int64_t hsh, int32_t h2_off);
int bot_spmm_dot_halves_f16(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                            const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* x, int64_t ldx, int64_t hsx, const float* w,
                            const int32_t* wperm, const float* y, int64_t ldy, int64_t hsy, int32_t H, int32_t D, const float* hscale, uint16_t* hout,
                            int64_t ldh, int64_t hsh, int32_t h2_off, float* dot_out, float* partial, bot_stream_t stream);
int bot_gemm_halves3_nt2_f32(int64_t m, int64_t n, int64_t k, const float* scale_a, const float* scale_a2, int64_t k_split, const float* scale_b,
                             const uint16_t* A, int64_t lda, int64_t a2_off, const uint16_t* B, int64_t ldb, int64_t b2_off, int32_t b_layout, float* C,
                             int64_t ldc, int32_t mode, bot_stream_t stream);
/* v18: the reduce pass of a fused BatchNorm / ReLU / dropout epilogue's backward (bot_bn_act_bwd_reduce_f32: 1 GB read per hidden layer at
 * config 2) as a BY-PRODUCT of the NT product that writes that epilogue's incoming gradient (bot_amd/nn/fused.py: the next layer's
 * `d h = d out . W^T`, backward of src/no-sampling/models.py:490-492 feeding the backward of :726-731).  With C = dy [m, n] and the
 * epilogue's input x [m, n] (n = the BatchNorm width F), the tile epilogue of bot_gemm_halves3_nt3_f32 forms, per stored element,
 *     g = dy * dropout_factor(seed, r, c) * [relu: weight_c xhat + bias_c > 0],   xhat = (x - mean_c) invstd_c
 * and leaves per 256-row tile t the partials  part[(2 t + 0) n + c] = sum_r g,  part[(2 t + 1) n + c] = sum_r g xhat  and (pmax != NULL)
 * pmax[(2 t + 0) n + c] = max_r |g|,  pmax[(2 t + 1) n + c] = max_r |xhat|  - the workspace layout of the reduce pass with one row block per
 * tile: ceil(m / 256) blocks (bot_gemm_halves3_nt_bn_rows(k): 256 when the product of piece width k takes this form - k a multiple of 64,
 * BOT_NT_KERNEL not 128x64 - else 0: the caller keeps the pass).  Finished by
 *   bot_bn_act_bwd_reduce_partials_f32  sum_g / sum_gx [F] from `part` (blocks added in order, in double: deterministic)
 *   bot_bn_bwd_bound_partials_f32       bot_bn_bwd_bound_f32 from `pmax`
 * The mask is the Philox function of (seed, r, c) the forward used (a quad of output columns = a quad of the mask).  x rows: 8-byte aligned,
 * pitch ldx >= n even; n even.  bn == NULL: bot_gemm_halves3_nt2_f32. */
typedef struct bot_bn_bwd_stats {
    const float* x;              /* [m, n] the epilogue's input (pre-BatchNorm), row pitch ldx */
    int64_t ldx;
    const float* mean;           /* [n] */
    const float* invstd;         /* [n] */
    const float* weight;         /* [n] or NULL (1) */
    const float* bias;           /* [n] or NULL (0) */
    int32_t relu;
    float p;                     /* dropout probability of the epilogue, 0: none */
    uint64_t seed;
    const uint64_t* seed_offset; /* optional device word mixed into the seed (hipGraph replays), as in bot_bn_act_fwd_f32 */
    float* part;                 /* [ceil(m / 256)][2][n] */
    float* pmax;                 /* [ceil(m / 256)][2][n] or NULL */
} bot_bn_bwd_stats_t;
int32_t bot_gemm_halves3_nt_bn_rows(int64_t k);
int bot_gemm_halves3_nt3_f32(int64_t m, int64_t n, int64_t k, const float* scale_a, const float* scale_a2, int64_t k_split, const float* scale_b,
                             const uint16_t* A, int64_t lda, int64_t a2_off, const uint16_t* B, int64_t ldb, int64_t b2_off, int32_t b_layout, float* C,
                             int64_t ldc, const bot_bn_bwd_stats_t* bn, int32_t mode, bot_stream_t stream);
/* d h recomputed in the apply (the DEFERRED form of the v18 by-product, for products with a short reduction).  When nobody but that
 * epilogue's backward reads C - the consumer layer took its input as halves only - storing C [m, n] and reading it back in the apply pass
 * is traffic the result does not need (2 x 508 MB for the config-2 output layer).  The product is launched twice instead:
 *   bot_gemm_halves3_nt_bn_reduce_f32  bot_gemm_halves3_nt3_f32 with `bn`, except that C is not stored (C may be NULL, ldc is not read): part / pmax
 *                                      come out bit for bit (the same accumulation, the same fold over the 8-row groups of a tile);
 *   bot_gemm_halves3_nt_bn_apply_f32   the same main loop over the same operands (the tile's values are the bits the store would have
 *                                      written), and in the epilogue bot_bn_act_bwd_apply_f32 / _halves_f32 on them with the finished sums:
 *       dx = weight invstd (g - sum_g / total_count - xhat sum_gx / total_count)
 *     as fp32 (dx, pitch lddx; optional) and / or the LEFT halves operand [h1 | 2^11 h2] of hscale[0] dx (hout; optional; head blocks of hD
 *     columns every hDP, second half h2_off behind the first, padding columns untouched), max|dx| into absmax_slots (optional).  sum_g =
 *     sum_gx = NULL: running statistics.  The operations and their order are those of bn_act_bwd_apply_kernel as compiled for gfx950, so dx
 *     and the halves are the bits that pass writes from the stored C.  bn->part / pmax are not used.
 * Refused with BOT_E_RANGE: a piece width k for which bot_gemm_halves3_nt_bn_rows(k) is not 256, or above
 * bot_gemm_halves3_nt_bn_deferred_max_k() = 256 halves; an odd n; x (or dx) rows that are not 8-byte aligned.  The bound on k is where the
 * second main loop stops paying: it costs 6 m n k flops of fp16 MFMA plus a second read of A, about 0.1 ms per 128 halves of k at the
 * config-2 shape (m = 169 343, n = 750), against the 2 x 4 m n bytes it saves, about 0.3 ms there at the 3 - 3.5 TB/s these passes reach -
 * break-even near k = 400, and the next piece width in use (1 536, the hidden layers) is far beyond it: those keep the storing form. */
int32_t bot_gemm_halves3_nt_bn_deferred_max_k(void);
int bot_gemm_halves3_nt_bn_reduce_f32(int64_t m, int64_t n, int64_t k, const float* scale_a, const float* scale_a2, int64_t k_split, const float* scale_b,
                                      const uint16_t* A, int64_t lda, int64_t a2_off, const uint16_t* B, int64_t ldb, int64_t b2_off, int32_t b_layout,
                                      float* C, int64_t ldc, const bot_bn_bwd_stats_t* bn, bot_stream_t stream);
int bot_gemm_halves3_nt_bn_apply_f32(int64_t m, int64_t n, int64_t k, const float* scale_a, const float* scale_a2, int64_t k_split, const float* scale_b,
                                     const uint16_t* A, int64_t lda, int64_t a2_off, const uint16_t* B, int64_t ldb, int64_t b2_off, int32_t b_layout,
                                     const bot_bn_bwd_stats_t* bn, const float* sum_g, const float* sum_gx, double total_count, float* dx, int64_t lddx,
                                     const float* hscale, uint16_t* hout, int64_t ldh, int32_t h2_off, int32_t hD, int32_t hDP, uint32_t* absmax_slots,
                                     bot_stream_t stream);
int bot_bn_act_bwd_reduce_partials_f32(const float* part, int32_t nblk, int32_t F, float* sum_g, float* sum_gx, bot_stream_t stream);
int bot_bn_bwd_bound_partials_f32(int32_t F, const float* pmax, int32_t nblk, const float* sum_g, const float* sum_gx, double total_count,
                                  const float* weight, const float* invstd, uint32_t* absmax_slots, bot_stream_t stream);
/* both in ONE launch, for one rank (no cross-rank reduction of the sums in between): sum_g / sum_gx as _reduce_partials forms them, then the
 * bound from them (batch_stats = 0: eval statistics, the sums do not enter it) */
int bot_bn_bwd_partials_finish_f32(const float* part, const float* pmax, int32_t nblk, int32_t F, float* sum_g, float* sum_gx, int32_t batch_stats,
                                   double total_count, const float* weight, const float* invstd, uint32_t* absmax_slots, bot_stream_t stream);
/* v17: a RIGHT operand in FRAGMENT-MAJOR layout (b_layout = 1 of bot_gemm_halves3_nt2_f32; ldb / b2_off unused): the 16 bytes lane l of an
 * MFMA fragment holds - row 16 t + (l & 15), columns 32 s + 8 (l >> 4) .. + 7 - at halves ((t T + s) 64 + l) 8, T = piece / 32, h1 in the
 * first region, h2 ceil(n / 16) T 512 halves behind it: the 64 lanes of a fragment load read one contiguous KB (the NT kernel pays for the
 * bytes a CU pulls from its L2 by their address pattern: profiles/r05_nt64.txt).  out: 2 * ceil(n / 16) * (piece / 32) * 512 halves, 16-byte
 * aligned; piece a multiple of 64; rows beyond n and columns beyond F are zeros. */
int bot_halves_split_frag_f16(const float* x, int64_t ldx, int64_t n, int32_t F, const float* scale, uint16_t* out, int32_t piece, bot_stream_t stream);
int bot_gemm_halves3_tn2_f32(int64_t n_rows, int64_t k, int64_t p, int64_t kp, int64_t pp, const float* scale_x, const float* scale_d, const float* scale_d2,
                             int64_t p_split, const uint16_t* X, int64_t ldx, int64_t x2_off, const uint16_t* D, int64_t ldd, int64_t d2_off, float* out,
                             int64_t ldo, float* workspace, int32_t mode, bot_stream_t stream);

/* v16: GROUPED forms of the two products above — the column tiles (NT) / output tiles (TN) of ONE launch are a host-side list, each entry
 * with its own operand columns and output block.  They carry the aggregate-first GAT layer (fused.py:_GATHiddenAggFirst; models.py:490-492,
 * :547, :558-560 reordered by linearity): per head h  rst_h = [x | z_h] [Wres_h | W_h]^T  (one reduction over two column ranges of the
 * left operand), d z_h = d rst_h W_h, and the weight gradients d W_h = d rst_h^T z_h, d Wres = d rst^T x as blocks of one launch.
 *
 *   nt_grouped  groups[g] = (b_row0, n_valid, a_col0, a_col1, k_steps, c_off):
 *     C[r * ldc + c_off + j] = scale_a[1] scale_b[1] * sum_{t < k_steps} sum_{i < 32} A3[r, (t < k_seg ? a_col0 : a_col1) + 32 t + i] . B3[b_row0 + j, 32 t + i]
 *     for r < m, j < n_valid <= 256 (A3 . B3: the three products a1 b1 + a1 b2 + a2 b1; a1 at the given column, 2^11 a2 a2_off behind it;
 *     b1 at column 32 t + i of B's row, b2 b2_off behind it).  1 <= n_groups <= 12; a_col0, a_col1 multiples of 8; b_rows = rows of B.
 *     Optional epilogue (the eval-mode layer, models.py:726-734): col_scale / col_shift (either may be NULL), indexed by c_off + j — groups
 *     that write the columns of ONE [m, ldc] matrix —, then ReLU if `relu`, then max|C| into `absmax_slots` (NULL: none):
 *     C = relu?(C * col_scale + col_shift).
 *   tn_grouped  tiles[i] = (x_col0, k_valid, d_col0, p_valid, out_off, ldo, transposed):
 *     out[out_off + k * ldo + p] = scale_x[1] scale_d[1] * sum_n X3[n, x_col0 + k] . D3[n, d_col0 + p]   for k < k_valid <= 192, p < p_valid <= 192
 *     (transposed != 0: out[out_off + p * ldo + k]); 1 <= n_tiles <= 16; workspace: bot_gemm_halves3_tn_grouped_workspace_floats(n_rows, n_tiles) floats.
 * `groups` / `tiles` are HOST arrays of 6 resp. 7 int64 per entry (copied into the kernel arguments). */
int bot_gemm_halves3_nt_grouped_f32(int64_t m, int64_t b_rows, const float* scale_a, const float* scale_b, const uint16_t* A, int64_t lda,
                                    int64_t a2_off, const uint16_t* B, int64_t ldb, int64_t b2_off, float* C, int64_t ldc, int32_t n_groups,
                                    const int64_t* groups, int32_t k_seg, const float* col_scale, const float* col_shift, int32_t relu,
                                    uint32_t* absmax_slots, int32_t mode, bot_stream_t stream);
/* v17: nt_grouped with column statistics of the stored values as a by-product (BatchNorm's batch statistics without a pass over the
 * layer's output): per 256-row tile t and output column c = c_off + j, stats_pivot[t stats_F + c] = the tile's FIRST stored value of the
 * column (v19: written by the launch - a pivot inside the data keeps the sum of squares from cancelling for columns whose mean is far
 * from zero; v17/18 read one caller-given pivot per column), stats_part[(2 t + 0) stats_F + c] = sum over the tile's rows of
 * (C - pivot), [(2 t + 1) stats_F + c] the sum of squares, stats_minmax likewise the column minimum / maximum - ceil(m / 256) row blocks in
 * the layout of bot_bn_stats_halves_partials_f32, which combines the tiles exactly (in double) into mean / invstd / running statistics /
 * the epilogue's halves scale.  All three NULL: no statistics (= bot_gemm_halves3_nt_grouped_f32). */
int bot_gemm_halves3_nt_grouped2_f32(int64_t m, int64_t b_rows, const float* scale_a, const float* scale_b, const uint16_t* A, int64_t lda,
                                     int64_t a2_off, const uint16_t* B, int64_t ldb, int64_t b2_off, float* C, int64_t ldc, int32_t n_groups,
                                     const int64_t* groups, int32_t k_seg, const float* col_scale, const float* col_shift, int32_t relu,
                                     uint32_t* absmax_slots, float* stats_part, float* stats_minmax, float* stats_pivot, int32_t stats_F,
                                     int32_t mode, bot_stream_t stream);
/* (v19) part / minmax [nblk][2][F], pivot [nblk][F], nblk = ceil(n / 256) row blocks of 256 rows (the last one shorter). */
int bot_bn_stats_halves_partials_f32(const float* part, const float* minmax, int32_t nblk, const float* pivot, int64_t n, int32_t F, float eps, float momentum,
                                     float* mean, float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                     const float* weight, const float* bias, float p, float* hscale, float* bound_workspace, bot_stream_t stream);
int64_t bot_gemm_halves3_tn_grouped_workspace_floats(int64_t n_rows, int32_t n_tiles);
int bot_gemm_halves3_tn_grouped_f32(int64_t n_rows, const float* scale_x, const float* scale_d, const uint16_t* X, int64_t ldx, int64_t x2_off,
                                    const uint16_t* D, int64_t ldd, int64_t d2_off, float* out, int32_t n_tiles, const int64_t* tiles,
                                    float* workspace, int32_t mode, bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * v14: the train step's glue (csrc/step.hip) — what src/no-sampling/run.py does around the model with a dozen small tensor ops per
 * step, as four launches.  Deterministic (fixed-order reductions, no atomics); Philox streams as in bot_bn_act_fwd_f32 (`seed`,
 * optional device word `seed_offset` for hipGraph replays).
 *
 *   label_split   run.py:256-267.  keep_i = mask[i] (uint8, may be NULL) or u_i < mask_rate.  use_labels != 0: code[train_idx[i]] =
 *                 keep_i ? label : -1 (the node's label is an input feature this step, run.py:259-263) and wn[train_idx[i]] = !keep_i
 *                 (it is a prediction node); use_labels == 0: wn[train_idx[i]] = keep_i (run.py:265-267).  count[0] = sum of the wn written.
 *                 `code` / `wn` are [N] arrays the CALLER initialised once to -1 / 0 (entries of non-training nodes never change);
                 `workspace`: 128 int32 words (per-workgroup counts, folded in slot order: two launches).
 *   build_input   `add_labels` (run.py:240-243) + the stack's input dropout (models.py:711) in one pass:
 *                 out[n, :] = dropout_p([feat[n, :F] | onehot(code[n])[:C]]), survivors scaled by 1 / (1 - p); C may be 0.
 *   node_loss     run.py:229-236 per node and its gradient: ce = logsumexp(x) - x[label]; kind 0 logit: y = ce, 1 loge: y = log(eps + ce)
 *                 - log eps, 2 savage: y = (1 - exp(-ce))^2;  y_out[n] = wn[n] > 0 ? y : 0 (entries n .. n_pad - 1 are zeroed: pad to a
 *                 multiple of 64 for the fixed-order sum that follows);  dx[n, c] = wn[n] > 0 ? y'(ce) (softmax(x)[c] - [c == label]) /
 *                 count[0] : 0 (dx may be NULL); C <= 128.  Labels of nodes with wn = 0 may be placeholders (clamped into range, never used).
 *   rmsprop_step  torch.optim.RMSprop (run.py:331-333; momentum 0, not centered) for n_tensors <= 48 parameters in ONE launch:
 *                 g += weight_decay p; sq = alpha sq + (1 - alpha) g^2; p -= lr g / (sqrt(sq) + eps).  `params` / `grads` / `square_avg`
 *                 / `numel` are HOST arrays (of device pointers / element counts), copied into the launch; lr_dev (may be NULL): a device
 *                 scalar that overrides `lr` (captured steps).
 * ------------------------------------------------------------------------------------------- */
int bot_label_split_f32(const int64_t* train_idx, int64_t n_train, const int64_t* labels, int64_t ldl, const uint8_t* mask, float mask_rate,
                        uint64_t seed, const uint64_t* seed_offset, int32_t use_labels, int32_t* code, float* wn, float* count, int32_t* workspace,
                        bot_stream_t stream);
int bot_build_input_f32(const float* feat, int64_t ldf, int64_t n, int32_t F, int32_t C, const int32_t* code, float p, uint64_t seed,
                        const uint64_t* seed_offset, float* out, int64_t ldo, bot_stream_t stream);
/* build_input_reuse: build_input for a label-reuse pass (run.py:274-279).  Row n's label columns are onehot(code[n]) if code[n] >= 0; else
 * softmax(pred[n, :C]) (fp32, max-subtracted, one expf per class) if reuse == NULL or reuse[n] != 0 - a node without an input label this step:
 * masked-out training, validation, test; else zeros (a node in none of the sets: the reference never writes its columns).  Input dropout
 * exactly as build_input (same Philox blocks and words): with no row on the softmax branch the two outputs are equal bit for bit.
 * 1 <= C <= 128 (BOT_E_RANGE otherwise); NULL code / pred / out -> BOT_E_NULL.  One launch, no workspace, no atomics. */
int bot_build_input_reuse_f32(const float* feat, int64_t ldf, int64_t n, int32_t F, int32_t C, const int32_t* code, const uint8_t* reuse,
                              const float* pred, int64_t ldp, float p, uint64_t seed, const uint64_t* seed_offset, float* out, int64_t ldo,
                              bot_stream_t stream);
int bot_node_loss_f32(const float* x, int64_t ldx, int64_t n, int32_t C, const int64_t* labels, int64_t ldl, const float* wn, const float* count,
                      int32_t kind, float eps, float* y, int64_t n_pad, float* dx, int64_t lddx, bot_stream_t stream);
/* node_loss_weighted: node_loss with a per-node weight lw (float32 [n]) and the weight total of the prediction nodes, wsum[0] = the sum of
 * lw over wn > 0, in the place of count (GraphSAINT's loss normalisation as a self-normalised weighted mean):
 *   y_out[n] = wn[n] > 0 ? lw[n] y : 0;   dx[n, c] = wn[n] > 0 ? lw[n] y'(ce) (softmax(x)[c] - [c == label]) / wsum[0] : 0.
 * The same kernel form, loss kinds, padding and placeholder-label handling; with lw = 1 and wsum = count the outputs equal node_loss's bit
 * for bit.  1 <= C <= 128, kind in 0..2, n_pad >= n (BOT_E_RANGE otherwise); NULL x / labels / wn / lw / wsum / y -> BOT_E_NULL. */
int bot_node_loss_weighted_f32(const float* x, int64_t ldx, int64_t n, int32_t C, const int64_t* labels, int64_t ldl, const float* wn, const float* lw,
                               const float* wsum, int32_t kind, float eps, float* y, int64_t n_pad, float* dx, int64_t lddx, bot_stream_t stream);
int bot_rmsprop_step_f32(int32_t n_tensors, float* const* params, const float* const* grads, float* const* square_avg, const int64_t* numel,
                         float lr, const float* lr_dev, float alpha, float eps, float weight_decay, bot_stream_t stream);

/* solution index (hipblaslt_ext::getIndexFromAlgo) and search time in ms of the kernel the last gemm_halves call used; what
 * tools/tune_halves_gemm.py records into bot_amd/tuning/halves_gemm.json and passes back as `algo_index` (-1: none) */
int bot_gemm_halves_last_algo(int32_t* index, float* ms);
int bot_gemm_halves_library_version(int32_t* compiled, int32_t* runtime);

/* ---------------------------------------------------------------------------------------------
 * Small-K projections: C[m,n] = (accumulate ? C : 0) + A[m,k] op(B), k <= 256, m huge — the per-head products of the
 * aggregate-before-project layer (W_h . sum_u a x_u: src/no-sampling/models.py:490-492 applied after :547, the reordering
 * GraphConv does at :377-385) and its residual / score columns (:519-522, :553-557).  fp32 operands are split in registers into
 * three bf16 terms each (exactly; bf16 has fp32's exponent range, so no scale), six bf16 MFMA products per tile
 * (a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1, dropped terms <= 2^-24 relative), fp32 accumulation: fp32-GEMM accuracy without
 * any pass over the operands.  b_is_kn: B is stored [k, n] (1) or [n, k] (0, nn.Linear's weight layout), row-major with
 * pitch ldb.  batch > 1: strided batches (element strides), e.g. the H heads writing side by side into the columns of one matrix.
 * ------------------------------------------------------------------------------------------- */
int bot_skinny_gemm_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int32_t b_is_kn, float* C, int64_t ldc, int64_t m,
                        int32_t n, int32_t k, int32_t accumulate, int32_t batch, int64_t stride_a, int64_t stride_b, int64_t stride_c,
                        bot_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Weight gradients of the small-K projections: out[kx, ky] = sum_r X[r, kx] Y[r, ky] over the n node rows, kx / ky a few hundred
 * (d W_r = h^T d out2, d W_i = d x_i^T z_i of the aggregate-before-project layer; the backward of the nn.Linear calls at
 * src/no-sampling/models.py:490-492, 553-557).  Exact fp32 MFMA (v_mfma_f32_32x32x2_f32: with the reduction index on the rows both
 * operands are read as coalesced row segments, no transposition), one workgroup per 256 x 192 output block and row chunk with the rows
 * staged through LDS, transpose_out: out[ky, kx] instead (put the wider operand first: blocks are 256 of X by 192 of Y), per-chunk
 * partials in `workspace` (bot_tn_gemm_workspace_floats) added in chunk order: deterministic.  batch > 1: element strides.
 * ------------------------------------------------------------------------------------------- */
/* v16: the same product for an X of a handful of columns (kx <= 32, ky <= 256: the attention columns of the merged gradient against the
 * layer input): plain fp32 FMAs, one thread per column of Y, per-workgroup partials added in workgroup order.
 * workspace: bot_tn_narrow_workspace_floats(n, kx, ky) floats. */
int64_t bot_tn_narrow_workspace_floats(int64_t n, int32_t kx, int32_t ky);
int bot_tn_narrow_f32(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t n, int32_t kx, int32_t ky, float* out, int64_t ldo,
                      int32_t transpose_out, float* workspace, bot_stream_t stream);
int64_t bot_tn_gemm_workspace_floats(int64_t n, int32_t kx, int32_t ky, int32_t batch);
int bot_tn_gemm_f32(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t n, int32_t kx, int32_t ky, float* out, int64_t ldo,
                    int32_t transpose_out, int32_t batch, int64_t stride_x, int64_t stride_y, int64_t stride_out, float* workspace,
                    bot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BOT_GNN_H */
