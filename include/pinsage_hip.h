/*
 * pinsage_hip.h -- C-ABI of the MI355X (gfx950) PinSage convolution engine.
 *
 * The reference (MatejBevec/gcn-song-embeddings) is pure Python; its train-step
 * path calls into DGL (g.successors) and ATen CPU ops.  These entry points are
 * what a maintainer binds (ctypes stub in INTEGRATION.md) to replace those
 * call sites.  Plain pointers and sizes only; every device pointer is HIP
 * device memory (e.g. a torch tensor's data_ptr()), every `stream` a
 * hipStream_t.  Functions return 0 on success or a negative pinsage_status;
 * pinsage_last_error() gives the message of the calling thread's last failure.
 * No call synchronises the stream unless its comment says so.
 */
#ifndef PINSAGE_HIP_H
#define PINSAGE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum pinsage_status {
  PINSAGE_OK = 0,
  PINSAGE_ERR_HIP = -1,
  PINSAGE_ERR_ARG = -2,
  PINSAGE_ERR_WORKSPACE = -3,
  PINSAGE_ERR_GRAPH = -4, /* zero-degree node met by a walk (reference: torch.randint(0) raises) */
  PINSAGE_ERR_INDEX = -5, /* id out of range (reference: IndexError in h[nodeset]) */
};

/* ------------------------------------------------------------------ library */
int pinsage_version(void);
const char* pinsage_last_error(void);
/* number of visible HIP devices (0 when none); never fails */
int pinsage_device_count(void);

/* ------------------------------------------------------------------ RNG (host, no GPU needed)
 * Opaque MT19937 state with torch's CPU-generator semantics.  Replaces the
 * global generator the reference draws from in pinsage_model.py:42,45,50 and
 * pinsage_training.py:58,74 (torch.randint / torch.rand / torch.randperm).
 * torch_state is torch.get_rng_state() (5056 bytes). */
int pinsage_mt_state_bytes(void);
int pinsage_mt_from_torch(void* mt, const uint8_t* torch_state, int64_t nbytes);
int pinsage_mt_to_torch(const void* mt, uint8_t* torch_state, int64_t nbytes);
int pinsage_mt_seed(void* mt, uint64_t seed);
int pinsage_mt_skip(void* mt, int64_t n_draws);
int pinsage_mt_draws(void* mt, uint32_t* out, int64_t n);
/* torch.randperm(n)[:k] (pinsage_training.py:58,74): writes the first k entries
 * of the Fisher-Yates permutation and advances mt by the full n-1 draws. */
int pinsage_mt_randperm_prefix(void* mt, int64_t n, int64_t k, int64_t* out);

/* sample_batch with easy negatives (pinsage_training.py:53-77, 89-97) on the
 * host: positives is [P][2] int64, batch_out is [B][3] int64 (query, positive,
 * negative).  Consumes exactly the draws the reference does.  nodeset_out
 * (nullable, capacity 3B) receives batch.flatten().unique() (sorted), its
 * length in *n_nodeset. */
int pinsage_sample_batch_easy(void* mt, const int64_t* positives, int64_t n_pos_pairs,
                              int64_t n_items, int64_t batch_size, int64_t* batch_out,
                              int64_t* nodeset_out, int64_t* n_nodeset);

/* Batch sampler runtime (native data loader for PinSage.train's batch loop).
 * Holds positives [P][2] int64 (must stay alive and unchanged) and draws the
 * batch that the torch CPU generator state `state` (torch.get_rng_state()
 * bytes) yields: batch_out [B][3], nodeset_out (nullable, capacity 3B) =
 * batch.flatten().unique(), state_after = the generator state after the
 * reference's draws.  With speculate != 0 the batch starting at state_after is
 * drawn next on a worker thread and used by the next call iff its state is
 * byte-identical -- results are always exactly pinsage_sample_batch_easy's.
 * Returns 1 when the speculative draw was used, 0 when drawn synchronously. */
typedef struct pinsage_batch_sampler pinsage_batch_sampler;
int pinsage_batch_sampler_create(const int64_t* positives, int64_t n_pos_pairs, int64_t n_items,
                                 int64_t batch_size, pinsage_batch_sampler** out);
void pinsage_batch_sampler_destroy(pinsage_batch_sampler* s);
int pinsage_batch_sampler_next(pinsage_batch_sampler* s, const uint8_t* state, int64_t nbytes,
                               int64_t* batch_out, int64_t* nodeset_out, int64_t* n_nodeset,
                               uint8_t* state_after, int speculate);
/* The batch the worker drew speculatively for the NEXT request (from the
 * generator state the last pinsage_batch_sampler_next handed back), without
 * consuming it: waits for the worker, copies rows x 3 int64 ids into
 * batch_out and returns rows (0 if there is no finished draw or it exceeds
 * max_rows).  The next request still verifies its start state; a caller that
 * acts on a peeked batch (the trainer computes that batch's frontier ahead)
 * must compare it with the batch it is finally given. */
int pinsage_batch_sampler_peek(pinsage_batch_sampler* h, int64_t* batch_out, int64_t max_rows);

/* ------------------------------------------------------------------ sampler (device)
 * do_random_walks (pinsage_model.py:32-53).  CSR: indptr int64 [n_all+1],
 * indices int32 [E], successors in edge-insertion order (DGL g.successors,
 * pinsage_model.py:41,44).  sources int64 [n_src], trace int32 [n_src][n_hops].
 *
 * MT mode: `mt` (host state) is advanced by exactly 3*n_hops*n_src draws, as
 * the reference consumes.  `ws` is device scratch of pinsage_walk_mt_workspace
 * bytes (the raw MT words of one round of sources; smaller workspaces run in
 * more rounds).  Synchronises the stream (host prepares each round's chunk
 * states while the previous round runs). */
int64_t pinsage_walk_mt_workspace(int64_t n_src, int64_t n_hops);
int pinsage_walk_mt(const int64_t* indptr, const int32_t* indices, int64_t n_all,
                    const int64_t* sources, int64_t n_src, int64_t n_hops, float alpha, void* mt,
                    void* ws, int64_t ws_bytes, int32_t* trace, void* stream);
/* Philox mode: draws for (source position src_base+i, hop j) = Philox4x32-10
 * (key=seed, counter={j, pos_lo, pos_hi, offset}).  Synchronises the stream to
 * check for zero-degree nodes. */
int pinsage_walk_philox(const int64_t* indptr, const int32_t* indices, int64_t n_all,
                        const int64_t* sources, int64_t n_src, int64_t n_hops, float alpha,
                        uint64_t seed, uint32_t offset, int64_t src_base, int32_t* trace,
                        void* stream);

/* visit_prob.topk(k, 1) on the walks (pinsage_model.py:96-107): counts visits
 * per source, zeroes the source's own column, selects the top k with the exact
 * libstdc++ tie order of torch's CPU topk.  Outputs (any may be null):
 *   w_out f64 [n_src][k] = count / n_hops, nb_out int64 [n_src][k]   (reference dtypes)
 *   wn_out f32 [n_src][t_norm], nb32_out int32 [n_src][t_norm]: the first
 *     t_norm columns with weights divided by their row sum (device table)
 * dense_scratch: device bytes >= pinsage_visit_topk_scratch(n_src, n_all, k). */
int64_t pinsage_visit_topk_scratch(int64_t n_src, int64_t n_all, int64_t k);
int pinsage_visit_topk(const int32_t* trace, const int64_t* sources, int64_t n_src,
                       int64_t n_hops, int64_t n_all, int64_t k, void* dense_scratch,
                       double* w_out, int64_t* nb_out, float* wn_out, int32_t* nb32_out,
                       int64_t t_norm, void* stream);
/* Fused walk + visit counting + top-k (the SURVEY's ppr_topk): replaces
 * do_random_walks -> sample_neighborhood -> visit_prob.topk(k, 1)
 * (pinsage_model.py:32-53, 88-107) in sample_neighborhood_topt and
 * precompute_neighborhoods_topt (:103-132), and PersPageRank.knn
 * (baselines.py:114-151).  The walk's trace stays in LDS (never in HBM); outputs
 * as pinsage_visit_topk.  mt != null: MT19937 mode (host state advanced by
 * 3*n_hops*n_src draws, exactly the reference's consumption); mt == null:
 * Philox mode keyed by (seed, hop, src_base + i, offset), the same draws as
 * pinsage_walk_philox.  Only the partial_sort regime (k * 64 <= n_all); the
 * nth_element regime of tiny graphs goes through pinsage_visit_topk.
 * ws: device bytes >= pinsage_ppr_topk_workspace(n_src, n_hops, mt != null)
 * (smaller workspaces run in rounds).  Synchronises the stream (zero-degree
 * check: the reference's torch.randint(0) raises). */
int64_t pinsage_ppr_topk_workspace(int64_t n_src, int64_t n_hops, int rng_mt);
int pinsage_ppr_topk(const int64_t* indptr, const int32_t* indices, int64_t n_all,
                     const int64_t* sources, int64_t n_src, int64_t n_hops, float alpha, int64_t k,
                     void* mt, uint64_t seed, uint32_t offset, int64_t src_base, void* ws,
                     int64_t ws_bytes, double* w_out, int64_t* nb_out, float* wn_out,
                     int32_t* nb32_out, int64_t t_norm, void* stream);
/* sample_neighborhood_topt_early_stop (pinsage_model.py:55-86): pinsage_ppr_topk
 * whose walk from a source ends at the hop where the stop_np-th node reaches
 * stop_nv visits (visits to the source itself count; stop_np < 1 or stop_nv < 1
 * never stops).  With L the hops taken, the weights are count / L over the
 * first L hops, and the top k is taken over n_items columns (the reference's
 * visit_counts is [n, n_items]): only the partial_sort regime, k * 64 <=
 * n_items, else PINSAGE_ERR_ARG.  n_hops <= 2048.  A zero-degree node or an id
 * >= n_items among the hops taken gives PINSAGE_ERR_GRAPH (the message names
 * the first such source).  hops_out (nullable) int32 [n_src] device: L per
 * source.  Philox mode draws as pinsage_ppr_topk (a stop only truncates), one
 * wave per source.  MT19937 mode (mt != null) is for parity with the reference,
 * not for speed: a stopped source consumes 3 L - 1 words (the break comes
 * before that hop's torch.rand), an unstopped one 3 n_hops, so each source
 * starts where the one before stopped and one wave walks them in order; the
 * host state is left advanced by the words consumed, also written to
 * *words_out (nullable, host; 0 in Philox mode).  ws: device bytes >=
 * pinsage_ppr_topk_early_stop_workspace(n_src, n_hops, mt != null) (smaller
 * workspaces run in rounds, each starting where the last one ended).
 * Synchronises the stream. */
int64_t pinsage_ppr_topk_early_stop_workspace(int64_t n_src, int64_t n_hops, int rng_mt);
int pinsage_ppr_topk_early_stop(const int64_t* indptr, const int32_t* indices, int64_t n_all, int64_t n_items,
                                const int64_t* sources, int64_t n_src, int64_t n_hops, float alpha, int64_t k,
                                int64_t stop_np, int64_t stop_nv, void* mt, uint64_t seed, uint32_t offset,
                                int64_t src_base, void* ws, int64_t ws_bytes, double* w_out, int64_t* nb_out,
                                float* wn_out, int32_t* nb32_out, int64_t t_norm, int32_t* hops_out,
                                int64_t* words_out, void* stream);
/* pinsage_ppr_topk (Philox mode) over n_seg consecutive segments of sources in
 * one call: segment i = sources[seg_start[i] .. seg_start[i+1]) is keyed by
 * (seg_seed[i], hop, seg_base[i] + j, offset), so each segment draws exactly
 * what its own pinsage_ppr_topk call would.  Serves the train step's model
 * calls on the fly (pinsage_model.py:142-154, called at :183-185 once per
 * call), one walk per segment and one top-k pass and zero-degree check for
 * all.  seg_start / seg_seed / seg_base are host arrays (n_seg + 1, n_seg,
 * n_seg); ws >= pinsage_ppr_topk_workspace(seg_start[n_seg], n_hops, 0).
 * Synchronises the stream. */
int pinsage_ppr_topk_segments(const int64_t* indptr, const int32_t* indices, int64_t n_all,
                              const int64_t* sources, int64_t n_seg, const int64_t* seg_start,
                              const uint64_t* seg_seed, const int64_t* seg_base, int64_t n_hops,
                              float alpha, int64_t k, uint32_t offset, void* ws, int64_t ws_bytes,
                              double* w_out, int64_t* nb_out, float* wn_out, int32_t* nb32_out,
                              int64_t t_norm, void* stream);
/* ------------------------------------------------------------------ on-the-fly step (device)
 * relevant_nodes_per_layer (pinsage_model.py:142-154) for a train step's three
 * model calls (pinsage_training.py:183-185), all sizes on the device (no host
 * synchronisation: the on-the-fly step is captured whole).  Philox draws: call
 * c, fly layer k (0 = top) walks with key seeds[c * n_layers + k] and numbers
 * its sources from 0, as pinsage_ppr_topk_segments.  batch int64 [B][3]; call
 * c's node v is c * n + v in every table and position; tables nbt / wnt
 * (host arrays of n_layers device pointers, engine layer order: 0 = bottom)
 * [rows_cap >= 3 n + x_cap][T], rows of every layer's nodes written; virtual
 * nodes 3 n + j (j < *n_x <= x_cap, x_cap >= 3 B) are the earlier occurrences
 * of ids repeated inside a call (the last occurrence owns the id's row).
 * tab_ptrs: device array of 2 n_layers pointers (the nbt, then the wnt of
 * every engine layer).  pos_ids [3 B]: the engine's positions (3 i + c);
 * ids_xo [x_cap]: virtual node j's real node; fx (nullable) [3 n + x_cap][ld_x]:
 * the virtual rows j get feats[ids_xo[j] % n].  err[0] != 0x7f7f7f7f: a walk
 * met a zero-degree node; err[1] != 0: a drawn id >= n (the reference raises).
 * ws: pinsage_fly_workspace_bytes, initialised once by pinsage_fly_init_workspace. */
int64_t pinsage_fly_workspace_bytes(int64_t n, int64_t B, int64_t n_layers, int64_t T, int64_t n_hops);
int pinsage_fly_init_workspace(void* ws, int64_t n, int64_t B, int64_t n_layers, int64_t T, int64_t n_hops,
                               void* stream);
int pinsage_fly_sample(const int64_t* indptr, const int32_t* indices, int64_t n_all, const int64_t* batch,
                       int64_t B, int64_t n, int64_t n_layers, int64_t T, int64_t n_hops, float alpha,
                       const uint64_t* seeds, void* ws, int64_t ws_bytes, int32_t* const* nbt, float* const* wnt,
                       int32_t** tab_ptrs, int64_t rows_cap, int64_t* pos_ids, int* n_x, int64_t* ids_xo,
                       int64_t x_cap, const float* feats, int64_t ld_f, int64_t d, float* fx, int64_t ld_x,
                       int* err, void* stream);
/* The sampler's two error words into the host ring slot (*ctr % R) at err_off
 * (the captured on-the-fly step reports them there; the host reads them when
 * it next waits for that slot). */
int pinsage_fly_publish_err(const int* err, void* ring, int64_t slot_bytes, int64_t R, const int64_t* ctr,
                            int64_t err_off, void* stream);
/* Refuse the captured on-the-fly step's optimizer update when its sampling
 * failed (err[0] / err[1] as pinsage_fly_sample sets them): err[2] becomes a
 * sticky halt word (the host clears it after raising), and a halted step's
 * Adam coefficients get bc2 = coef[1] = 0, which every fused Adam kernel takes
 * as "leave parameters and moments untouched" -- the reference raises before
 * optimizer.step() (pinsage_model.py:25, pinsage_training.py:188-191). */
int pinsage_fly_gate_adam(int* err, float* coef, void* stream);
/* sample_neighborhood (pinsage_model.py:88-101): dense f64 [n_src][n_all]. */
int pinsage_visit_dense(const int32_t* trace, const int64_t* sources, int64_t n_src,
                        int64_t n_hops, int64_t n_all, double* dense, void* stream);

/* ------------------------------------------------------------------ frontier (device)
 * relevant_nodes_per_layer_precomp (pinsage_model.py:156-168) for the API:
 * one step nodes_out = unique(cat(nb[nodeset, :T].flatten(), nodeset)), sorted.
 * nb_table int32 [n_items][ld]; nodes_out int32 capacity >= n*(T+1) (and
 * <= n_items); *count_out (device int) receives the size.  ws: device bytes >=
 * pinsage_frontier_workspace(n_items). */
int64_t pinsage_frontier_workspace(int64_t n_items);
int pinsage_frontier_step(const int64_t* nodeset, int64_t n, const int32_t* nb_table, int64_t ld,
                          int64_t T, int64_t n_items, void* ws, int32_t* nodes_out,
                          int32_t* count_out, void* stream);
/* After pinsage_frontier_step on ws (same nodeset, table, T, n_items): the
 * index table local_idx int32 [n][T] with nodes_out[local_idx[f][t]] ==
 * nb[nodeset[f]][t] -- the rows of the unique set the convolution's slots
 * read (weighted_agg's loc), from the set's bitmap ranks. */
int pinsage_frontier_local_idx(const int64_t* nodeset, int64_t n, const int32_t* nb_table, int64_t ld, int64_t T,
                               int64_t n_items, const void* ws, int32_t* local_idx, void* stream);

/* ------------------------------------------------------------------ kernels exposed for tests
 * fp32 MFMA GEMM: C[M][N] = A[M][K] * W[N][K]^T (+bias) (leaky_relu if act),
 * A rows gathered by a_idx (nullable) -- nn.Linear on gathered rows
 * (pinsage_model.py:196,201). */
int pinsage_linear(const float* A, int64_t lda, const int32_t* a_idx, int64_t M, int64_t K,
                   const float* W, const float* bias, int64_t N, int act, float* C, int64_t ldc,
                   void* stream);
/* (the train-step engine's handle, see "train-step engine" below) */
typedef struct pinsage_engine pinsage_engine;
/* The train-step engine's frontier plan, for tests that read it back: the
 * workspace byte offsets of what pinsage_engine_frontier builds beside the
 * sets that pinsage_engine_offsets_t already locates.  Per layer l (index 0 =
 * bottom; |S_l|, |N_l| live entries, from count_S / count_N):
 *   self_src int32 [|S_l|]     row of S_l[f] in S_{l-1} (layer 0: the id itself)
 *   q_src    int32 [|N_l|]     row of N_l[u] in S_{l-1} (layer 0: the id itself)
 *   loc      int32 [|S_l|][T]  rank of nb[S_l[f]][t] in N_l
 *   wloc     f32   [|S_l|][T]  wn[S_l[f]][t], copied bit for bit
 * and the batch positions grouped by their top-set rank:
 *   rank_off   int32 [|S_top| + 1]  rank r's positions are pos_sorted[rank_off[r]
 *                                   .. rank_off[r + 1]); rank_off[0] = -1: absent
 *                                   (more than 16384 positions)
 *   pos_sorted int32 [n_ids]        positions by (pos_rank, position)
 * A struct of its own: pinsage_engine_offsets_t keeps its size for callers
 * compiled against it.  Entries of layers >= n_layers are 0. */
typedef struct {
  int64_t self_src[8], q_src[8], loc[8], wloc[8];
  int64_t rank_off, pos_sorted;
} pinsage_engine_plan_offsets_t;
int pinsage_engine_plan_offsets(const pinsage_engine* e, pinsage_engine_plan_offsets_t* out);
/* The head's and the loss's buffers, for tests that read them back (and write
 * Z or garbage into Gp before a loss): workspace byte offsets, rows = |S_top|
 * live rows (count_S of the top layer), out = the configuration's out_dim:
 *   H1      f32 [rows][out]     lrelu(y G1^T + b1)
 *   dP1     f32 [rows][out]     (dZ G2) * lrelu'(H1)
 *   dp_top  f32 [rows][out]     the top conv layer's dp (pre-activation gradient)
 *   nrm_top f32 [rows]          the top conv layer's row norms ||lrelu(.)||
 *   G       f32 [3][cap][out]   per call (query / positive / negative) and rank, the
 *                               summed loss cotangent of the rank's positions
 *   Kc      i32 [3][cap]        per call and rank, the number of positions
 *   Gp      f32 [max_pos][out]  a repeated rank's cotangent rows by position
 *   cap     the top set's capacity: the row stride of G and Kc (not an offset)
 * G and Kc are zero over their whole capacity outside a loss .. backward pair.
 * A struct of its own, as pinsage_engine_plan_offsets_t. */
typedef struct {
  int64_t H1, dP1, dp_top, nrm_top, G, Kc, Gp, cap;
} pinsage_engine_head_offsets_t;
int pinsage_engine_head_offsets(const pinsage_engine* e, pinsage_engine_head_offsets_t* out);
/* General form of the same GEMM, for per-configuration tests and
 * microbenchmarks: C = op(A) op(B) with A K-major ([M][K], rows gathered by
 * a_idx) or M-major ([K][M], k-rows gathered), B K-major ([N][K]) or N-major
 * ([K][N], k-rows gathered by b_idx); epi 0 store, 1 accumulate, 3 split-K
 * slabs C[splits][M][N]; cfg -1 picks the tile by size, 0..2 forces one;
 * stream_k -1 chooses by size, 0 disables, 1 forces the stream-K schedule
 * (in-launch combine of tiles cut between workgroups; scratch is owned by
 * the library). */
/* Weight gradient of an nn.Linear weight over a device-side row count
 * (the AddmmBackward of pinsage_model.py:196-201 / 208-210):
 *   dst[M][N] = A^T [B || B2]  (A [K][M] row-major; B rows gathered by b_idx
 *   when set, columns >= N1 from B2 -- torch.cat along N), dst_b[M] = column
 *   sums of A (nullable), K = *K_dev (nullable: K_max rows).  Long-K form
 *   (wgrad.hip): 64 x 64 tiles, K cut into `splits` runs (0: by size) that
 *   are combined inside the launch in a fixed order (deterministic); with
 *   adam_p set, torch.optim.Adam is applied to the slice (adam_* pointers in
 *   dst's layout, coef = {lr / (1 - b1^t), sqrt(1 - b2^t)} on the device).
 *   M, N, N1 multiples of 64.  scratch: pinsage_wgrad_scratch_bytes(M, N)
 *   bytes, zeroed once before the first call (its tickets reset themselves). */
int64_t pinsage_wgrad_scratch_bytes(int64_t M, int64_t N);
int pinsage_wgrad(int64_t M, int64_t N, const int* K_dev, int64_t K_max, const float* A, int64_t lda,
                  const float* B, int64_t ldb, const int32_t* b_idx, int64_t N1, const float* B2, int64_t ldb2,
                  float* dst, int64_t ld_dst, float* dst_b, int splits, void* scratch, float* adam_p,
                  float* adam_m, float* adam_v, float* adam_pb, float* adam_mb, float* adam_vb,
                  const float* coef, double beta1, double beta2, float eps, void* stream);
/* The same weight gradient with both operands given as their hi / mid / lo
 * bf16 planes (pinsage_split_planes: A3 [3][K][M], B3 [3][rows][N] with plane
 * strides a3_ps / b3_ps and row strides lda / ldb elements, B rows gathered
 * by b_idx): no conversions in the k loop.  Weights are bitwise the fp32
 * form's 4-wave launch (PINSAGE_KW_WAVES=4) on the planes' source matrices;
 * dst_b sums the planes' value (H + M) + L.  The layer-0 Q weight gradient
 * (pinsage_model.py:201's AddmmBackward) in the engine. */
/* Measurement only (tools/wgrad_bench.py): the weight-gradient launch with a
 * timing-only k loop -- probe 1: the DMAs without the products, 2: the products
 * without the DMAs, 3: 2 without the split, 4: the k loop without the split.
 * The results are WRONG by construction; nothing in the engine calls it. */
int pinsage_wgrad_probe(int64_t M, int64_t N, const int* K_dev, int64_t K_max, const float* A, const float* B,
                        const int32_t* b_idx, float* dst, float* dst_b, int splits, void* scratch, int probe,
                        void* stream);
int pinsage_wgrad_planes(int64_t M, int64_t N, const int* K_dev, int64_t K_max, const uint16_t* A3, int64_t a3_ps,
                         int64_t lda, const uint16_t* B3, int64_t b3_ps, int64_t ldb, const int32_t* b_idx,
                         float* dst, int64_t ld_dst, float* dst_b, int splits, void* scratch, void* stream);
int pinsage_gemm_ex(int64_t M, int64_t N, int64_t K, int a_kmajor, int b_kmajor, const float* A,
                    int64_t lda, const int32_t* a_idx, const float* B, int64_t ldb,
                    const int32_t* b_idx, float* C, int64_t ldc, const float* bias, int act,
                    int epi, int splits, int cfg, int stream_k, void* stream);
/* Product arithmetic of the fp32 GEMMs with K-major operands (the Q / W
 * projections of the forward, the kNN dot products): 0 = v_mfma_f32_32x32x2_f32
 * (exact fp32 FMA chains); 1 (default; PINSAGE_GEMM_PREC overrides at load) =
 * each fp32 operand split exactly into hi + mid + lo bf16 (|residual| <= 2^-26
 * |x|), the six products down to 2^-18 of hi*hi on v_mfma_f32_32x32x16_bf16
 * with fp32 accumulation: fp32-level error at 2.67x the fp32 MFMA rate.
 * Process-wide; other GEMMs always use fp32 MFMA. */
int pinsage_gemm_set_prec(int prec);
int pinsage_gemm_get_prec(void);
/* hi / mid / lo bf16 planes of a row-major fp32 matrix W[rows][cols] (row
 * stride ldw floats): out[3][rows][cols] as uint16 bf16 bits, the exact split
 * the split-bf16 GEMM does in registers (cols % 8 == 0, ldw % 4 == 0). */
int pinsage_split_planes(const float* W, int64_t rows, int64_t cols, int64_t ldw, uint16_t* out,
                         void* stream);
/* pinsage_linear's product (K-major A rows gathered by a_idx, W[N][K]) under
 * split-bf16 arithmetic with W given ALSO as its pre-split planes (from
 * pinsage_split_planes(W, N, K, ...): row stride ldws == K elements, plane
 * stride N*K; other strides are rejected): the kernel converts A only.
 * Bitwise equal to the in-register split for cfg 0 and 3 (other cfg values,
 * -1 included, may run the in-register form; the result is the same). */
int pinsage_linear_split_b(const float* A, int64_t lda, const int32_t* a_idx, int64_t M, int64_t K,
                           const float* W, const uint16_t* W_planes, int64_t ldws,
                           const float* bias, int64_t N, int act, float* C, int64_t ldc, int cfg,
                           void* stream);
/* max_margin_loss (pinsage_training.py:31-41) of outputs given per position,
 * Z f32 [3][B][d] (q, pos, neg calls; d <= 256 dividing 1024), with the train
 * step's own kernels and reduction order (pinsage_engine_loss): scal f32[4] =
 * {loss, 0, sum |z_q|^2, variance of the z_q}, G f32 [3][3B][d] = the loss
 * cotangent of position (c, b) at row G[c][c*B + b] (other rows zero).  Equal
 * rows give the step's loss bits.  scratch: pinsage_triplet_loss_scratch_bytes
 * bytes, 16-B aligned.  The micro-batched step's loss. */
int64_t pinsage_triplet_loss_scratch_bytes(int64_t B, int64_t d);
int pinsage_triplet_loss(const float* Z, int64_t B, int64_t d, float margin, float* G, void* scratch, float* scal,
                         void* stream);
/* Interleaved split-bf16 table of src[rows][K] (K % 16 == 0, ld % 4 == 0):
 * row r at out + r * ldo (bf16 elements, ldo % 8 == 0, ldo >= 3K) holds K/16
 * stages of six 16-B chunks -- hi, mid, lo bf16 of the stage's 16 values, 8
 * per chunk -- the exact split the GEMM does in registers.  The input feature
 * table is split once (features do not change during training), W_Q per step. */
int pinsage_split_ilv(const float* src, int64_t ld, int64_t rows, int64_t K, uint16_t* out, int64_t ldo,
                      void* stream);
/* C[m][0..N) = act(A[a_idx[m]] . W[n] + bias[n]) from an interleaved table of
 * A (rows gathered by a_idx) and W [N][K] either as its interleaved table
 * (W_ilv, pinsage_split_ilv) or, W_ilv null, fp32 split in registers: bitwise
 * pinsage_linear's split-bf16 product on the same 128 x 128 tiles, every
 * gathered row's 16-k stage one contiguous 96-B read.  M static or *M_dev <=
 * M_max.  The layer-0 Q projection (pinsage_model.py:201). */
int pinsage_linear_ilv(const uint16_t* A_ilv, int64_t lda_ilv, const int32_t* a_idx, int64_t M, const int* M_dev,
                       int64_t M_max, int64_t K, const float* W, const uint16_t* W_ilv, int64_t ldw_ilv,
                       const float* bias, int64_t N, int act, float* C, int64_t ldc, void* stream);
/* agg[f] = sum_t w[f][t] * q[loc[f][t]]  (weights already normalised;
 * pinsage_model.py:202). */
int pinsage_weighted_agg(const float* q, int64_t hid, const int32_t* loc, const float* w,
                         int64_t n_rows, int64_t T, float* agg, void* stream);
/* The transpose of that aggregation -- the backward of pinsage_model.py:202 with
 * respect to the q rows, through the LeakyReLU that produced them: for each q
 * row u in [0, *n_q_dev)
 *   dpq[u] = lrelu'(q[u]) * sum over the slots (f, t) with loc[f][t] == u of
 *            w[f][t] * dagg[f]
 * by the engine's own launches in the engine's order: the CSR transpose of the
 * slot table by q row with its chunk list (<= 16 slots per chunk) and the
 * canonical order of every q row's pairs (sorted by source row f), then the
 * chunk kernel.  mode 0: rows split over several chunks are summed by the
 * combine kernel; mode 1 (hid <= 512): by the fan-in-8 tree inside the chunk
 * kernel.  Both sum a row in a fixed order (bitwise reproducible).
 * The counts are device-side below static capacities, as in the engine:
 * *n_rows_dev <= n_rows_max source rows, *n_q_dev <= n_q_max q rows (the
 * capacities size the scratch and the grids, and choose the scan kernel).
 * loc int32 / w f32 [*n_rows_dev][T], 1 <= T <= 64; dagg f32 rows of stride
 * ld_dagg >= hid (a multiple of 4); q, dpq f32 [*n_q_dev][hid], hid % 4 == 0.
 * Preconditions the kernels do NOT check: every loc value lies in
 * [0, *n_q_dev), and the T entries of a row of loc are distinct (a q row's
 * source rows are distinct -- see pinsage_engine_set_tensors; a repeated
 * (u, f) pair leaves slots of the sorted pair list unwritten, whose stale
 * contents are then used as row indices into dagg).
 * A q row that occurs in no slot has no chunk: its dpq row is NOT written (the
 * engine's frontier only holds q rows that occur in a slot).
 * dpq_planes (nullable; mode 1 only): the result as hi / mid / lo bf16 planes
 * [3][plane_stride] (plane_stride >= n_q_max * hid elements, a multiple of 4;
 * row u at u * hid) -- bitwise pinsage_split_planes of the fp32 result --
 * INSTEAD of dpq, which is then not written.
 * scratch: pinsage_agg_transpose_scratch_bytes(n_rows_max, T, n_q_max, hid)
 * bytes (-1 for shapes the entry rejects), 256-B aligned: the per-row counters
 * cnt, the scan's block sums, off, cursor, cbase, the pair lists occ2 and
 * occ2b (the sort's second buffer), the chunk and split-row lists with their
 * counts, the split rows' partial sums and the tree's tickets, with the sizes
 * the engine carves per layer.  Zero it once before the first call: the scan
 * leaves cnt zero behind its read and the tree's tickets reset themselves, so
 * later calls on the same scratch (any mode) need no clearing.  Raises the
 * CSR kernels' dynamic-LDS limit on first use (not capturable). */
int64_t pinsage_agg_transpose_scratch_bytes(int64_t n_rows_max, int64_t T, int64_t n_q_max, int64_t hid);
int pinsage_agg_transpose(const int32_t* loc, const float* w, const int* n_rows_dev, int64_t n_rows_max, int64_t T,
                          const int* n_q_dev, int64_t n_q_max, const float* dagg, int64_t ld_dagg, const float* q,
                          int64_t hid, int mode, void* scratch, float* dpq, uint16_t* dpq_planes,
                          int64_t plane_stride, void* stream);

/* ConvLayer.forward after the Q projection (pinsage_model.py:195-210): for each
 * row f of n_rows,
 *   agg[f]  = sum_t w[f][t] * q[loc[f][t]]                     (:202, w normalised)
 *   y[f]    = normalize(lrelu([h[self_src[f]] || agg[f]] W^T + bias))   (:208-210)
 *   norms[f] = ||lrelu(.)||_2 (nullable)
 * the engine's kernel: the aggregate formed in registers and written out once,
 * the projection on split-bf16 MFMA.  h f32 [.][ldh], q f32 [q_rows][hid],
 * loc int32 / w f32 [n_rows][T], W f32 [out][d+hid], y f32 [n_rows][out],
 * agg f32 [n_rows][hid].  out == 128, 1 <= T <= 64, d + hid a multiple of 64,
 * d and hid multiples of 4.  W_planes (nullable device scratch of
 * 3 * out * (d + hid) uint16): where the 32-row tile runs (>= 16 rows per CU,
 * d + hid a multiple of 128, d a multiple of 32) W is split into it
 * (fragment-order bf16 planes) and the tile's gather runs pipelined against its
 * projection (the same y bitwise); null runs it unpipelined. */
int pinsage_conv_agg_project(const float* h, int64_t ldh, int64_t d, const int32_t* self_src,
                             const float* q, int64_t hid, int64_t q_rows, const int32_t* loc,
                             const float* w, int64_t n_rows, int64_t T, const float* W,
                             const float* bias, int64_t out, uint16_t* W_planes, float* y,
                             float* norms, float* agg, void* stream);

/* get_embeddings' row gather (pinsage_model.py:21-23): out[i][0..d) =
 * h[idx[i]][0..d), idx int64 (device).  Ids outside [0, n_h) give zero rows
 * (the reference raises IndexError: callers validate).  Its transpose
 * (the gradient, an index_add over repeated ids) is a pinsage_segment_wmean
 * over the CSR of idx, deterministic in summation order. */
int pinsage_gather_rows(const float* h, int64_t ldh, int64_t n_h, int64_t d, const int64_t* idx, int64_t n,
                        float* out, int64_t ldo, void* stream);
/* ConvLayer's W projection alone (pinsage_model.py:208-210):
 *   y[f] = normalize(lrelu([h[self_idx[f]][0..d) || agg[f]] W^T + bias)),
 *   norms[f] = ||lrelu(.)||_2
 * with the concat read in place (no concat buffer).  self_idx int32 nullable
 * (rows 0..n-1), W f32 [out][d+hid], d and hid multiples of 4.  out <= 128:
 * one launch (the GEMM's L2-norm epilogue); wider: the GEMM with bias +
 * LeakyReLU, then an in-place row normalisation. */
int pinsage_concat_linear_l2norm(const float* h, int64_t ldh, const int32_t* self_idx, int64_t n, int64_t d,
                                 const float* agg, int64_t ld_agg, int64_t hid, const float* W,
                                 const float* bias, int64_t out, float* y, float* norms, void* stream);
/* Backward of y = lrelu(p) / ||lrelu(p)|| (the autograd of pinsage_model.py:209-210):
 *   dp = lrelu'(y) * (dy - y (y . dy)) / norms     (y, dy, dp f32 [n][out]) */
int pinsage_norm_lrelu_backward(const float* y, const float* norms, const float* dy, int64_t n, int64_t out,
                                float* dp, void* stream);

/* ------------------------------------------------------------------ test entries
 * Nothing in the engine calls these: they expose the engine's own launches,
 * one at a time, to the tests (tests/test_gpu_gemm_forms.py,
 * tests/test_gpu_optimizer.py, tests/test_gpu_sampler_edges.py).  The GraphSAGE
 * baseline (baselines.SAGE) runs its dense products and its Adam steps on
 * pinsage_gemm_params and pinsage_adam.
 *
 * pinsage_gemm_params: one GEMM launch with every field of the library's
 * launch parameters (csrc/gemm.h GemmParams, which documents them) given by
 * the caller.  size = sizeof(pinsage_gemm_params_t) comes first (a mismatch is
 * refused); every other member is an int64_t or a pointer, flags are 0 / 1,
 * "unset" is -1 for K1, N1, cfg, stream_k and prec and 0 / NULL elsewhere
 * (splits and sk_min_units: at least 1).  In short, C = op(A) op(B):
 *   a_kmajor 1: A(m,k) = a[row(m) lda + k], row(m) = a_idx ? a_idx[m] : m; for
 *               k >= K1 >= 0 from a2 / lda2 / a2_idx at column k - K1
 *            0: A(m,k) = a[row(k) lda + m], row(k) = a_idx ? a_idx[k] : k
 *   b_kmajor 1: B(k,n) = b[n ldb + k]
 *            0: B(k,n) = b[row(k) ldb + n], row(k) = b_idx ? b_idx[k] : k; for
 *               n >= N1 >= 0 from b2 / ldb2 / b2_idx at column n - N1
 *   M = *M_dev <= M_max and K = *K_dev <= K_max when set (device-side counts;
 *   M_hint only picks the tile); rows >= M are not written.
 *   epi 0: c[dst(m) ldc + n] = f(acc + bias[n]), f = LeakyReLU when act, times
 *          lrelu'(mask[m ldm + n]) when mask (x > 0 ? 1 : 0.01); dst(m) =
 *          c_idx ? c_idx[m] : m.  With c2: columns n >= N1 go to
 *          c2[m ldc2 + n - N1] instead, by row m, stored plainly.
 *       1: the same added to c's previous value (c2's columns are still plain
 *          stores).  A mask with epi 1 is refused.
 *       2: v = lrelu(acc + bias), norms[m] = ||v||, c[dst(m) ldc + n] = v / ||v||
 *          (N <= 128).
 *       3: split-K slabs c[s][M][ldc] of the `splits` k ranges (K cut into runs
 *          of ceil(K / splits) rounded up to 32; an empty run's slab is zero),
 *          bias_part[s][M] = sums over the run's k of A(m,k) (M-major A).
 *   PRECONDITION the kernels do not check: c_idx names DISTINCT rows.  A tile's
 *   epilogue loads what it accumulates onto and stores without atomics, and
 *   tiles of different workgroups run concurrently: a repeated row loses
 *   updates.  The engine's self_src and q_src index the members of a set.
 *   sk_slab / sk_cnt / sk_cnt_len: stream-K scratch of the caller's,
 *   pinsage_gemm_sk_slab_floats() floats and sk_cnt_len ints, zeroed once (the
 *   tickets reset themselves); stream_k 1 forces the schedule where the launch
 *   allows it (cfg 1 or 2), 0 forbids it.  prec 0: fp32 MFMA, 1: split bf16,
 *   -1: the process default.  *ran_stream_k (nullable) = 1 if the launch ran
 *   the stream-K schedule, else 0. */
typedef struct {
  int64_t size;
  int64_t M, N, K;
  const int* M_dev;
  const int* K_dev;
  int64_t M_max, K_max;
  int64_t a_kmajor, b_kmajor;
  const float* a;
  int64_t lda;
  const int32_t* a_idx;
  int64_t K1;
  const float* a2;
  int64_t lda2;
  const int32_t* a2_idx;
  const float* b;
  int64_t ldb;
  const int32_t* b_idx;
  int64_t N1;
  const float* b2;
  int64_t ldb2;
  const int32_t* b2_idx;
  float* c;
  int64_t ldc;
  const int32_t* c_idx;
  float* c2;
  int64_t ldc2;
  float* bias_part;
  int64_t epi;
  const float* bias;
  int64_t act;
  const float* mask;
  int64_t ldm;
  float* norms;
  int64_t splits;
  int64_t M_hint;
  int64_t cfg;
  float* sk_slab;
  int* sk_cnt;
  int64_t sk_cnt_len;
  int64_t stream_k;
  int64_t sk_min_units;
  int64_t prec;
  const uint16_t* b_split;
  int64_t ldb_split;
  const uint16_t* a_ilv;
  const uint16_t* b_ilv;
  int64_t lda_ilv, ldb_ilv;
} pinsage_gemm_params_t;
int64_t pinsage_gemm_sk_slab_floats(void);
int pinsage_gemm_params(const pinsage_gemm_params_t* params, int* ran_stream_k, void* stream);
/* The split-K reduction of the weight gradients' fallback path:
 *   out[m ld + n] = sum over s < S of part[s stride + m N + n],
 *   bias_out[m]   = sum over s of bpart[s M + m]     (bpart / bias_out nullable)
 * in a fixed order: group g = 0..3 sums slabs g, g + 4, ... -- sixteen slabs
 * at a time as acc += (x0 + x1) + (x2 + x3), the rest one by one -- and the
 * groups combine as (g0 + g1) + (g2 + g3).  N, ld, stride multiples of 4,
 * 16-B aligned buffers.  With adam_p set, torch.optim.Adam's step is applied
 * to the slice from the reduced gradient (adam_p / adam_m / adam_v in out's
 * layout, adam_pb / adam_mb / adam_vb [M] with bias_out; coef as pinsage_adam). */
int pinsage_reduce_slabs(const float* part, int64_t S, int64_t stride, int64_t M, int64_t N, float* out,
                         int64_t ld, const float* bpart, float* bias_out, float* adam_p, float* adam_m,
                         float* adam_v, float* adam_pb, float* adam_mb, float* adam_vb, const float* coef,
                         double beta1, double beta2, float eps, void* stream);
/* One torch.optim.Adam step (_single_tensor_adam) on caller buffers p, g, m, v
 * f32 [n], 16-B aligned: coef (device) = {lr / (1 - beta1^t), sqrt(1 - beta2^t)};
 * coef[1] == 0 leaves p, m and v untouched. */
int pinsage_adam(float* p, const float* g, float* m, float* v, int64_t n, const float* coef, double beta1,
                 double beta2, float eps, void* stream);
/* pinsage_norm_lrelu_backward in the engine's form: the row count from *nrows
 * (device; <= n_max, which sizes the grid; null: n_max rows), and the zeroing
 * the engine folds into the launch: z[0, *z_rows * z_n) = 0 (z nullable) and
 * zi[0, zi_n) = 0 (zi nullable). */
int pinsage_norm_lrelu_backward_ex(const float* y, const float* norms, const float* dy, const int* nrows,
                                   int64_t n_max, int64_t out, float* dp, float* z, int64_t z_n,
                                   const int* z_rows, int* zi, int64_t zi_n, void* stream);
/* The fused sampler's two halves (tests/test_gpu_sampler_edges.py): what
 * pinsage_ppr_topk launches back to back, with the runs between them in caller
 * memory.  A source's runs are the (node id, visit count) pairs of its walk in
 * ascending id order, the source's own id dropped: runs uint32 [n_src][n_hops][2]
 * (row stride n_hops pairs), n_runs int32 [n_src] pairs written per source;
 * the pairs past n_runs[s] are not written.
 *
 * pinsage_walk_runs: the walk launch.  mt != null: MT19937 mode, the host state
 * advanced by 3*n_hops*n_src draws, ws device bytes >= pinsage_walk_mt_workspace(
 * n_src, n_hops) (one round; a smaller workspace is PINSAGE_ERR_WORKSPACE); mt ==
 * null: Philox mode keyed as pinsage_walk_philox (ws unused).  err: one device
 * int, set to 0x7f7f7f7f and then to the smallest index of a source whose walk
 * met a zero-degree node (PINSAGE_ERR_GRAPH; that source gets n_runs = 0 and
 * no runs, every other source its own).  n_hops <= 8192.  Synchronises.
 *
 * pinsage_runs_topk: the top-k launch over caller-supplied runs, outputs as
 * pinsage_visit_topk (each pair null or both set).  n_src_dev (nullable): n_src
 * is a capacity that sizes the grid and the live count is min(n_src,
 * *n_src_dev) on the device; rows at and past it are not written.
 * Preconditions the kernel does NOT check: per source ids strictly ascending,
 * counts >= 1 summing to <= n_hops, 0 <= n_runs <= n_hops.  k >= 1, n_hops <=
 * 8192, k + n_hops < 65536, t_norm in [1, k] with wn_out, and k small enough
 * for one source's heap (k | 1 words) to fit the 64 KB of LDS: a refused call
 * (PINSAGE_ERR_ARG) launches nothing.  There is no n_all: the row is as wide as
 * the partial_sort regime needs (k * 64 <= n_all, every id < n_all).
 * A source without runs (every hop came back to it): w_out is k zeros with ids
 * 0 .. k-1 in libstdc++'s order, and wn_out is 0 / 0 = NaN in every column, as
 * the reference's own division gives; pinsage_visit_topk writes the same bits.
 * Does not synchronise.
 *
 * pinsage_walk_runs_seg: the on-the-fly sampler's walk launch (Philox): n_calls
 * calls' sources sorted by call, seg int32 [n_calls + 1] (device) their segment
 * starts, call c keyed by seeds[c * key_stride] (device) and numbering its
 * sources from 0; a source is sources64[s] or sources32[s] (exactly one set)
 * minus c * id_unit.  n_src_cap sizes the grid; slots at and past seg[n_calls]
 * are not written.  err as pinsage_walk_runs.  Synchronises. */
int pinsage_walk_runs(const int64_t* indptr, const int32_t* indices, int64_t n_all, const int64_t* sources,
                      int64_t n_src, int64_t n_hops, float alpha, void* mt, uint64_t seed, uint32_t offset,
                      int64_t src_base, void* ws, int64_t ws_bytes, uint32_t* runs, int32_t* n_runs, int32_t* err,
                      void* stream);
int pinsage_runs_topk(const uint32_t* runs, const int32_t* n_runs, int64_t n_src, int64_t n_hops, int64_t k,
                      const int32_t* n_src_dev, double* w_out, int64_t* nb_out, float* wn_out, int32_t* nb32_out,
                      int64_t t_norm, void* stream);
int pinsage_walk_runs_seg(const int64_t* indptr, const int32_t* indices, int64_t n_all, const int64_t* sources64,
                          const int32_t* sources32, int64_t n_src_cap, const int32_t* seg, int64_t n_calls,
                          const uint64_t* seeds, int64_t key_stride, int64_t id_unit, int64_t n_hops, float alpha,
                          uint32_t offset, uint32_t* runs, int32_t* n_runs, int32_t* err, void* stream);

/* ------------------------------------------------------------------ step hand-off
 * (PinSage.train_batch, pinsage_training.py:181-214, as ONE graph launch per step)
 * pinsage_step_stage: copy nbytes at src_off of slot (*ctr % R) of a pinned host
 * ring (slot_bytes each) to dst, and 8 bytes at coef_off to coef_dst (if set);
 * offsets and sizes multiples of 8.  pinsage_step_publish: ring_out[*ctr % R2]
 * [0..n) = scal[0..n) (n <= 64), then *ctr += 1.  Both read the counter on the
 * device, so a captured step graph stages and publishes the step the host
 * wrote, without copies between launches. */
int pinsage_step_stage(const void* ring, int64_t slot_bytes, int64_t R, const int64_t* ctr,
                       int64_t src_off, int64_t nbytes, void* dst, int64_t coef_off, void* coef_dst,
                       void* stream);
int pinsage_step_publish(const float* scal, int64_t n, float* ring_out, int64_t R2, int64_t* ctr,
                         void* stream);
/* Measurement only (bench.py's per-kernel timing pass): one wave that holds the
 * stream for `us` microseconds (0..1e6) of the constant 100 MHz clock, so the
 * launches the host queues behind it run back to back and events around them
 * time the kernels rather than the host's enqueue gaps. */
int pinsage_stream_hold(int64_t us, void* stream);

/* The host side of one captured train step (pinsage_training._FusedStep) in
 * one call -- the per-step work of pinsage_training.py:181-191's loop body
 * before the device runs it.  ring: the pinned hand-off ring [R][slot_bytes]
 * whose slot holds the step's ids (off_ids), the predicted next ids
 * (off_next) and the Adam coefficients (off_coef, 2 f32).  Per parity p
 * (workspace), three hipGraphExec_t of torch captures: gf (stage + frontier),
 * gm (the step), ga (the step + the next batch's frontier in the other
 * workspace).  pinsage_stepper_step: waits for the slot's previous step,
 * writes coef, launches gf unless the batch equals the ids whose frontier the
 * previous step computed ahead, then ga with `next` (the sampler's predicted
 * next batch, nullable) or gm, and records the slot's event.  batch / next:
 * n_ids int64 host ids (ids outside [0, n_items): kErrIndex, nothing
 * launched).  info (nullable) int64[2] = {ahead hit, step index}. */
typedef struct pinsage_stepper pinsage_stepper;
int pinsage_stepper_create(void* ring, int64_t R, int64_t slot_bytes, int64_t off_ids, int64_t off_next,
                           int64_t off_coef, int64_t max_ids, int64_t n_items, pinsage_stepper** out);
void pinsage_stepper_destroy(pinsage_stepper* s);
int pinsage_stepper_set_graphs(pinsage_stepper* s, int p, void* gf, void* gm, void* ga);
/* host nanoseconds spent blocked on ring slots so far (the device behind the host) */
int64_t pinsage_stepper_wait_ns(const pinsage_stepper* s);
/* out[0 .. n) of {ns blocked on ring slots, ns inside hipGraphLaunch, ns inside
 * pinsage_stepper_step, steps, ahead hits} (host accounting of the native path) */
int pinsage_stepper_stats(const pinsage_stepper* s, int64_t* out, int n);
/* resume from the trainer's eager path: next parity, step counter, no pending frontier */
int pinsage_stepper_sync_state(pinsage_stepper* s, int parity, int64_t nstep);
int pinsage_stepper_step(pinsage_stepper* s, const int64_t* batch, int64_t n_ids, const float* coef,
                         const int64_t* next, void* stream, int64_t* info);

/* ------------------------------------------------------------------ lib/gnns MEAN aggregator
 * GNN_model.aggregate, agg_func 'MEAN' (lib/gnns/GNNs_unsupervised.py:537-588):
 * mask.mm(embed_matrix) with the dense [F, U] mask kept as a CSR.  For each
 * segment i in [0, n_seg), entries j in [seg_ptr[i], seg_ptr[i+1]):
 *   out[i, :] = sum_j w[j] * h[cols[j], :] / den_i
 * den_i = max(sum_j |w[j]|, 1e-12) (F.normalize(p=1)) if normalize, else 1.
 * h f32 [n_h][ldh], out f32 [n_seg][ldo], seg_ptr int64 [n_seg + 1], cols int32,
 * w f32 (device).  Entries whose col is outside [0, n_h) are skipped (the
 * caller validates).  The backward (dH = mask^T dOut) is the same call over the
 * transposed CSR with pre-normalised weights and normalize = 0. */
int pinsage_segment_wmean(const float* h, int64_t ldh, int64_t n_h, int64_t d, const int64_t* seg_ptr,
                          const int32_t* cols, const float* w, int64_t n_seg, int normalize, float* out,
                          int64_t ldo, void* stream);

/* ------------------------------------------------------------------ lib/gnns GAT aggregator
 * GNN_model.aggregate with gat=True (lib/gnns/GNNs_unsupervised.py:449-465,
 * 555-567): a softmax over each node's whole neighbourhood of
 * leaky_relu(att([h_own || h_nb]), 0.2) * sqrt(edge count), then mask.mm(h);
 * here an edge softmax fused with the row gather, no [F, U] mask and no
 * gathered [nnz, d] buffers.  Segment i has entries j in [seg_ptr[i],
 * seg_ptr[i+1]) with hrow[j] (int32 row of h) and c[j] >= 0; own[i] is the h
 * row of the segment's node; a = [a_l | a_r] f32 [2 d] (att.weight[0]):
 *   e_ij = s_l[own_i] + s_r[hrow_j],  s_l[u] = a_l . h[u],  s_r[u] = a_r . h[u]
 *   m_ij = (e_ij > 0 ? e_ij : 0.2 e_ij) * c_ij
 *   kept: m_ij != 0, hrow_j and own_i in [0, n_h)
 *   p_ij = exp(m_ij - M_i) / sum_kept exp(m_ik - M_i),  M_i = max_kept m_ik
 *   out_i = sum_j p_ij h[hrow_j]          (nothing kept: p = 0, a zero row)
 * and for dout f32 [n_seg][lddo]:
 *   g_ij = dout_i . h[hrow_j],  gbar_i = sum_j p_ij g_ij
 *   de_ij = p_ij (g_ij - gbar_i) c_ij (e_ij > 0 ? 1 : 0.2),  s_i = sum_j de_ij
 *   dh[hrow_j] += p_ij dout_i + de_ij a_r,  dh[own_i] += s_i a_l
 *   da = [sum_i s_i h[own_i] | sum_ij de_ij h[hrow_j]]
 * All pointers are device pointers; seg_ptr, segT, own_ptr int64, the other
 * index arrays int32; 0 < d <= 2^20, n_h <= INT32_MAX, leading dimensions >=
 * d.  Rows are read 16 bytes at a time when d, the leading dimensions and the
 * base pointers allow it, else 4.  No atomics and fixed summation orders: two
 * identical calls give the same bits.  A refused call (PINSAGE_ERR_ARG)
 * launches nothing.
 *
 * node_scores: s_l[u], s_r[u] for u = rows[t], t < n_rows (rows null: u = t,
 *   n_rows <= n_h); other elements of s_l, s_r [n_h] are left alone.
 * forward: out [n_seg][ldo] and p [nnz] (every entry written, 0 where dropped).
 * backward_edges: de [nnz], s [n_seg] from the forward's p.
 * backward_rows: rows_u int32 [n_rows] ascending and unique, covering every
 *   in-range hrow and own; segT [n_rows + 1] over (entT, segofT) = the entries
 *   k with hrow[k] == rows_u[t] and their segments; own_ptr [n_rows + 1] over
 *   own_seg = the segments i with own[i] == rows_u[t].  Writes row rows_u[t]
 *   of dh [n_h][lddh] (the other rows are the caller's: zero them), coef
 *   [2 n_rows] and partial [pinsage_gat_partial_rows(n_rows)][2 d] (scratch)
 *   and da [2 d]. */
int64_t pinsage_gat_partial_rows(int64_t n_rows);
int pinsage_gat_node_scores(const float* h, int64_t ldh, int64_t n_h, int64_t d, const float* a, const int32_t* rows,
                            int64_t n_rows, float* s_l, float* s_r, void* stream);
int pinsage_gat_forward(const float* h, int64_t ldh, int64_t n_h, int64_t d, const int64_t* seg_ptr,
                        const int32_t* hrow, const float* c, const int32_t* own, int64_t n_seg, int64_t nnz,
                        const float* s_l, const float* s_r, float* out, int64_t ldo, float* p, void* stream);
int pinsage_gat_backward_edges(const float* h, int64_t ldh, int64_t n_h, int64_t d, const int64_t* seg_ptr,
                               const int32_t* hrow, const float* c, const int32_t* own, int64_t n_seg, int64_t nnz,
                               const float* s_l, const float* s_r, const float* p, const float* dout, int64_t lddo,
                               float* de, float* s, void* stream);
int pinsage_gat_backward_rows(const float* h, int64_t ldh, int64_t n_h, int64_t d, const float* a,
                              const int32_t* rows_u, int64_t n_rows, const int64_t* segT, const int32_t* entT,
                              const int32_t* segofT, const int64_t* own_ptr, const int32_t* own_seg, const float* p,
                              const float* de, const float* s, int64_t nnz, int64_t n_seg, const float* dout,
                              int64_t lddo, float* dh, int64_t lddh, float* coef, float* partial, float* da,
                              void* stream);

/* ------------------------------------------------------------------ cosine kNN
 * knn_from_emb (baselines.py:91-103) over cosine_sim_ab (baselines.py:69-77), the
 * evaluation consumer of the embeddings (eval.py:112-143 save_knn, k = 1000):
 * for each query row q (int64 ids in [0, n), validated by the caller)
 *   sim(q, j) = dot(emb[q], emb[j]) / (|emb[q]| |emb[j]| + eps), j in [0, n)
 * out_w f32 [nq][k] / out_n int64 [nq][k]: the k largest, sorted descending
 * (exact ties: lower index first).  The reference then drops column 0.
 * emb: f32 device rows of stride ld floats, 16-byte aligned (d % 4 == 0,
 * ld >= d and ld % 4 == 0: rows are read in 16-byte pieces; the ld - d floats
 * after a row are never read); 1 <= k <= min(n, 4096).  A refused call
 * (PINSAGE_ERR_ARG, PINSAGE_ERR_WORKSPACE) launches nothing.
 * scratch: device bytes >= pinsage_knn_scratch_bytes(n, rows) for some
 * batch of rows >= 1 (the dot products of one batch of queries live there;
 * larger scratch = fewer batches). */
int64_t pinsage_knn_scratch_bytes(int64_t n, int64_t batch_rows);
int pinsage_knn_cosine(const float* emb, int64_t n, int64_t d, int64_t ld, const int64_t* queries,
                       int64_t nq, int64_t k, float eps, void* scratch, int64_t scratch_bytes,
                       float* out_w, int64_t* out_n, void* stream);

/* ------------------------------------------------------------------ ranks of given rows
 * hit_rate / mrr (eval.py:227-250) over held-out pairs (q, pos) without kNN
 * lists: both are functions of one integer per pair, the rank of pos among all
 * n rows under pinsage_knn_cosine's order for q.  Query row u (queries[u], an
 * id that may repeat across rows) owns targets[grp_ptr[u] .. grp_ptr[u + 1]);
 * for each of them
 *   out_rank[i] = #{ j in [0, n) : key(j) > key(t) or (key(j) == key(t) and j < t) },  t = targets[i]
 * with key the order-preserving image of sim(q, j) as pinsage_knn_cosine
 * computes it (the same device function).  So for any k, column r of
 * pinsage_knn_cosine's row for q holds t exactly when out_rank == r < k; a
 * target is not counted against itself, and a target listed twice gets the
 * same rank twice.  Ranks are integer counts: the result is deterministic.
 * queries int64 [nu], targets int64 [np], out_rank int64 [np]: device (ids in
 * [0, n), validated by the caller); grp_ptr int64 [nu + 1]: HOST memory, checked
 * during the call and copied to the device on the stream (pageable memory is
 * staged before the call returns; keep page-locked memory until the stream has
 * run the call), from 0 to np, never decreasing, no group above
 * pinsage_rank_max_group() = 4096 targets (split a larger group by repeating
 * the query row).  emb, n, d, ld, eps as for pinsage_knn_cosine.  A refused
 * call (PINSAGE_ERR_ARG: those size and alignment conditions, grp_ptr not
 * starting at 0 / decreasing / not ending at np, a group above the capacity;
 * PINSAGE_ERR_WORKSPACE: scratch below pinsage_rank_scratch_bytes(n, 1))
 * launches nothing and leaves out_rank untouched.
 * scratch: device bytes >= pinsage_rank_scratch_bytes(n, rows) for some batch
 * of rows >= 1 (one batch: norms, one gathered-row GEMM, one counting pass of
 * n * 8 B per query row). */
int64_t pinsage_rank_scratch_bytes(int64_t n, int64_t batch_rows);
int64_t pinsage_rank_max_group(void);
int pinsage_rank_cosine(const float* emb, int64_t n, int64_t d, int64_t ld, const int64_t* queries,
                        int64_t nu, const int64_t* grp_ptr, const int64_t* targets, int64_t np, float eps,
                        void* scratch, int64_t scratch_bytes, int64_t* out_rank, void* stream);

/* ------------------------------------------------------------------ beyond-accuracy list metrics
 * The device work of compute_beyond_accuracy_table (eval.py:445-467).
 *
 * pinsage_row_inv_norms: inv[r] = 1 / sqrt(sum_c x[r][c]^2) over x f32 [n] rows
 * of d floats, row stride ld >= d (the ld - d floats after a row are never
 * read), IEEE square root and division (a squared norm that is a power of four
 * has an exact inverse); a zero row gives +inf.  The lengths of eval.py:259
 * (cosine_sim_mat), inverted once per table row instead of once per list slot.
 *
 * pinsage_list_intra_sim: what intra_diversity (eval.py:271-286) computes per
 * query before its mean: for row i of lists (int64 [nq] rows of stride ldk, the
 * first kc columns used, ids in [0, n))
 *   out[i] = | sum_{c < kc} inv[id_c] * feat[id_c][:] |^2 / (float)(kc * kc),
 * the mean of the kc x kc matrix of cosine_sim_mat (eval.py:255-264) over the
 * listed rows, its diagonal and repeated ids included.  NaN rule: a listed row
 * of zeros has inv = +inf, and inf * 0 makes that query's value NaN, as the
 * reference's 0 / 0 does (it has no eps); other queries are unaffected.  The
 * sum runs in slot order and the reduction order is fixed: two runs give the
 * same bits.  feat / inv as for pinsage_row_inv_norms (inv [n] from it).
 *
 * pinsage_list_pair_overlap: what inter_diversity (eval.py:288-312) needs per
 * sampled pair.  Set semantics: the reference marks one-hot columns, so a
 * repeated id counts once; scipy's cosine distance between two such rows is
 * 1 - |A & B| / sqrt(|A| |B|).  For pair p = (a, b) of pairs (int64 [np][2],
 * rows of lists in [0, nq), a == b allowed), A = set(lists[a][:kc]) and B
 * likewise:
 *   out[3 p] = |A|,  out[3 p + 1] = |B|,  out[3 p + 2] = |A & B|   (int32).
 * Ids lie in [0, n_ids), n_ids < 2^31; 1 <= kc <= pinsage_list_overlap_max_k()
 * = 4096.
 *
 * All pointers are device memory.  err (nullable): a device int set to 1 when
 * an id (or a pair's row) is out of range; the value is clamped so that no
 * access strays, and the caller raises.  A refused call (PINSAGE_ERR_ARG: a
 * null pointer other than err, kc < 1, kc > ldk, kc above the capacity,
 * ld < d, a size out of range) returns before any launch and leaves the
 * outputs untouched. */
int pinsage_row_inv_norms(const float* x, int64_t n, int64_t d, int64_t ld, float* inv, void* stream);
int pinsage_list_intra_sim(const float* feat, int64_t n, int64_t d, int64_t ld, const float* inv,
                           const int64_t* lists, int64_t nq, int64_t ldk, int64_t kc, float* out, int* err,
                           void* stream);
int64_t pinsage_list_overlap_max_k(void);
int pinsage_list_pair_overlap(const int64_t* lists, int64_t nq, int64_t ldk, int64_t kc, int64_t n_ids,
                              const int64_t* pairs, int64_t np, int32_t* out, int* err, void* stream);

/* ------------------------------------------------------------------ Jaccard co-occurrence neighbours
 * JaccardFast (baselines.py:194-220) without its n_tracks x n_tracks scipy
 * product.  The playlist-track membership relation is given as two CSRs with
 * duplicates removed (device arrays):
 *   t2c_ptr int64 [n_tracks + 1], t2c_idx int32: the collections of each track,
 *     ids in [0, n_cols);
 *   c2t_ptr int64 [n_cols + 1],  c2t_idx int32: the tracks of each collection,
 *     ids in [0, n_tracks), ASCENDING within a row (the kernel binary-searches).
 * deg[t] = t2c_ptr[t + 1] - t2c_ptr[t] is the reference's nbh_sizes.
 *
 * pinsage_cooc_counts: out int32 [nq][n_tracks],
 *   out[i][t] = #{ c : queries[i] in c and t in c },
 * the rows intersect_sizes[nodeset, :].toarray() of the reference.  The track
 * range is tiled through LDS in tiles of pinsage_cooc_tile() counters; every
 * element of out is written exactly once (no memset is needed) and the counts
 * are integer adds: two runs give the same bits.
 *
 * pinsage_cooc_jaccard: for each query q
 *   s(q, t) = float(co) / (float(deg[q] + deg[t] - co) + 1e-10f),  t in [0, n_tracks)
 * in fp32 with IEEE division, which is what torch computes for the reference's
 * intersect / (union + 1e-10) over int32 tensors (two tracks in no collection
 * score 0).  out_w f32 [nq][k] / out_n int64 [nq][k]: the k largest, sorted
 * descending, exact ties by ascending id (pinsage_knn_cosine's order and
 * selection kernel); a row with fewer than k non-zero scores is filled with the
 * lowest zero-score ids.  The reference then drops column 0.
 * 1 <= k <= min(n_tracks, 4096), n_tracks < 2^31.  scratch: 16-byte aligned
 * device bytes >= pinsage_cooc_scratch_bytes(n_tracks, rows) for some batch of
 * rows >= 1 (the int32 count rows of one batch of queries live there).
 *
 * queries int64 [nq] (device).  err (nullable): a device int set to 1 when a
 * query id is outside [0, n_tracks); the id is clamped so that no access
 * strays, and the caller raises.  A refused call (PINSAGE_ERR_ARG: a size out
 * of range, k outside its bounds, a null pointer other than err and the index
 * arrays of an empty relation; PINSAGE_ERR_WORKSPACE: scratch below one row)
 * returns before any launch and leaves the outputs untouched. */
int64_t pinsage_cooc_tile(void);
int64_t pinsage_cooc_scratch_bytes(int64_t n_tracks, int64_t batch_rows);
int pinsage_cooc_counts(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                        const int32_t* c2t_idx, int64_t n_tracks, int64_t n_cols, const int64_t* queries,
                        int64_t nq, int32_t* out, int* err, void* stream);
int pinsage_cooc_jaccard(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                         const int32_t* c2t_idx, int64_t n_tracks, int64_t n_cols, const int64_t* queries,
                         int64_t nq, int64_t k, void* scratch, int64_t scratch_bytes, float* out_w, int64_t* out_n,
                         int* err, void* stream);

/* The weighted form, behind the link-prediction indices of SimpleSimilarity
 * (baselines.py:153-191; Adamic-Adar).  The two CSRs are read as node ->
 * middle nodes and middle node -> nodes, in the layout above; for a graph's
 * own adjacency (the projected track graph) both are that adjacency.
 * wt int64 [n_cols] (device; null only where n_cols == 0) is a weight per
 * middle node:
 *   S(q, t) = sum of wt[c] over the middle nodes c adjacent to both q and t,
 * in 64-bit integer adds (wrapping; independent of the order, so two runs give
 * the same bits).  The track range is tiled through LDS in tiles of
 * pinsage_cooc_weighted_tile() 64-bit counters; no global atomic, no memset,
 * every output element is written exactly once.
 *
 * pinsage_cooc_weighted_sums: out int64 [nq][n_tracks], out[i][t] = S(queries[i], t).
 *
 * pinsage_cooc_weighted_knn: score(q, t) = float32(S(q, t)) * 2^-30 (the
 * int64 -> float32 conversion rounds to nearest even; the weights are 2^30
 * fixed point and the sums >= 0), out_w f32 [nq][k] / out_n int64 [nq][k]: the
 * k largest per query in pinsage_cooc_jaccard's order, by the same selection
 * kernel.  scratch: 16-byte aligned device bytes >=
 * pinsage_cooc_weighted_scratch_bytes(n_tracks, rows) for some batch of
 * rows >= 1 (the float score rows of one batch live there).
 *
 * Sizes, k, queries, err and refused calls as for pinsage_cooc_jaccard. */
int64_t pinsage_cooc_weighted_tile(void);
int64_t pinsage_cooc_weighted_scratch_bytes(int64_t n_tracks, int64_t batch_rows);
int pinsage_cooc_weighted_sums(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                               const int32_t* c2t_idx, int64_t n_tracks, int64_t n_cols, const int64_t* wt,
                               const int64_t* queries, int64_t nq, int64_t* out, int* err, void* stream);
int pinsage_cooc_weighted_knn(const int64_t* t2c_ptr, const int32_t* t2c_idx, const int64_t* c2t_ptr,
                              const int32_t* c2t_idx, int64_t n_tracks, int64_t n_cols, const int64_t* wt,
                              const int64_t* queries, int64_t nq, int64_t k, void* scratch, int64_t scratch_bytes,
                              float* out_w, int64_t* out_n, int* err, void* stream);

/* ------------------------------------------------------------------ implicit-feedback ALS
 * The fit behind ColTrackCfALS / TrackTrackCfALS (baselines.py:458-514), which
 * the reference takes from implicit.cpu.als.AlternatingLeastSquares: the model
 * of Hu, Koren and Volinsky solved row by row with the conjugate-gradient scheme
 * of Takacs et al.  The arithmetic below is this project's definition; parity
 * with that package's numbers is not claimed.
 *
 * pinsage_als_gram: G f32 [f][f] = Y^T Y + reg I for Y f32 [n][ld].  Fixed
 * summation order, no float atomics: the same bits on every run, symmetric bit
 * for bit, exact on small integers.
 *
 * pinsage_als_half: one half-iteration, rows X f32 [n_rows][ldx] solved in
 * place from fixed Y f32 [n_other][ldy] and G = pinsage_als_gram(Y).  The sparse
 * matrix is a CSR: ptr int64 [n_rows + 1], idx int32 (ids in [0, n_other)), val
 * f32 (> 0).  With c = alpha val the confidence, for each row u over its items i:
 *   x = X[u];  r = -G x + sum_i (c - (c - 1)(y_i . x)) y_i;  p = r;  rs = r . r
 *   if rs < 1e-20: X[u] stays as it is
 *   repeat cg_steps times:
 *     Ap = G p + sum_i (c - 1)(y_i . p) y_i
 *     a = rs / (p . Ap);  x += a p;  r -= a Ap;  rn = r . r
 *     if rn < 1e-20: break
 *     p = r + (rn / rs) p;  rs = rn
 *   X[u] = x
 * in fp32.  A row without items follows the same recurrence.  Row u reads X[u]
 * and Y only; only columns [0, f) of X are written (padding keeps its bits);
 * cg_steps == 0 launches nothing.  A row of at most pinsage_als_long_row() items
 * is solved by one wave, its item sums in CSR order; a longer one by a whole
 * workgroup, wave w summing the 64-item groups w, w + 8, ... in order and the 8
 * partial sums added in wave order.  The form depends on the row's length
 * alone: the output bits depend on the inputs only, not on the grid or the run.
 * Row r belongs to the block of rows r / pinsage_als_rows_per_block(); a
 * workgroup takes four consecutive blocks.
 *
 * All pointers are device memory.  err (nullable): a device int set to 1 when an
 * id is outside [0, n_other); the id is clamped so that no access strays, and the
 * caller raises.  A refused call (PINSAGE_ERR_ARG: f outside [4, 128] or
 * f % 4 != 0; a leading dimension below f or not a multiple of 4; Y, X or G
 * not 16-byte aligned or null; reg <= 0; alpha <= 0 or not finite;
 * cg_steps < 0; a count above INT32_MAX; n_other < 1) returns before any launch
 * and leaves X and G untouched. */
int64_t pinsage_als_rows_per_block(void);
int64_t pinsage_als_long_row(void);
int pinsage_als_gram(const float* Y, int64_t n, int64_t f, int64_t ld, float reg, float* G, void* stream);
int pinsage_als_half(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                     int64_t n_other, int64_t ldy, float* X, int64_t ldx, int64_t f, const float* G, float alpha,
                     int64_t cg_steps, int* err, void* stream);

/* ------------------------------------------------------------------ logistic matrix factorisation
 * Johnson, "Logistic Matrix Factorization for Implicit Feedback Data" (2014):
 * the algo="lmf" the reference takes from the implicit package.  The arithmetic
 * below is this project's definition, the paper's full-gradient AdaGrad ascent
 * without negative sampling; parity with that package's numbers is not claimed.
 *
 * R [n_users, n_items] is a CSR with values r > 0, c = alpha r.  Tables X
 * [n_users, f], Y [n_items, f], biases bx [n_users], by [n_items]; the score is
 * s_ui = x_u . y_i + bx_u + by_i.  The objective to MAXIMISE is
 *   L = sum_obs c s - sum_obs (1 + c) softplus(s) - sum_unobs softplus(s)
 *       - (reg / 2)(|X|^2 + |Y|^2)                     (biases not regularised)
 * One iteration updates every user row from (Y, by), then every item row from
 * the new (X, bx) with R^T as the CSR.  A half-iteration is Jacobi: every row
 * reads the old tables only.  Per row u, in fp32:
 *   D    = sum_all i sig(s_ui) y_i         dsum = sum_all i sig(s_ui)
 *   w_i  = c_ui sig(-s_ui)  for observed i       (= c (1 - sig(s)), no cancellation)
 *   g    = sum_obs w_i y_i - D - reg x_u   gb = sum_obs w_i - dsum
 *   h   += g^2 (elementwise)               hb += gb^2    (AdaGrad, start at 0)
 *   x_u += lr g / sqrt(1e-6 + h)           bx_u += lr gb / sqrt(1e-6 + hb)
 * sig is evaluated stably: for s >= 0 it is 1 / (1 + e^-s), otherwise
 * e^s / (1 + e^s); it is never NaN or Inf for finite s.
 *
 * pinsage_lmf_dense: D f32 [n_rows][ldd] and dsum f32 [n_rows] for every row of
 * X, bx against all of Y f32 [n_other][ldy], by.  One fused kernel on the
 * exact-f32 MFMA: no n_rows x n_other buffer exists.  A workgroup owns
 * pinsage_lmf_row_block() rows and walks all items in ascending order; no
 * atomics, the same bits on every run, and the bits of row u depend on x_u,
 * bx_u, Y and by only.  Columns [f, ld) are neither read nor written.
 *
 * pinsage_lmf_update: the rest of the recurrence, in place on X, bx, H f32
 * [n_rows][ldh], hb, from D and dsum of the old tables; CSR as pinsage_als_half.
 * s_i is recomputed for the observed cells from the old x_u as (x . y_i + bx) +
 * by_i; g = fma(-reg, x, sum - D), h = fma(g, g, h).  A row of at most
 * pinsage_lmf_long_row() items is taken by one wave, its item sums in CSR
 * order; a longer one by a whole workgroup, wave w summing the 64-item groups
 * w, w + 8, ... and the 8 partial sums added in wave order.  The form depends on
 * the row's length alone.  lr == 0 leaves X and bx bit for bit and still updates
 * H and hb.
 *
 * All pointers are device memory.  err (nullable): as pinsage_als_half.  A
 * refused call (PINSAGE_ERR_ARG: f outside [4, 128] or f % 4 != 0; a leading
 * dimension below f or not a multiple of 4; a table not 16-byte aligned or
 * null; a null bias, dsum or hb; alpha <= 0, reg < 0, lr < 0 or any not finite;
 * a count above INT32_MAX; n_other < 1) returns before any launch and leaves
 * every output untouched.  n_rows == 0 is accepted and launches nothing. */
int64_t pinsage_lmf_row_block(void);
int64_t pinsage_lmf_long_row(void);
int pinsage_lmf_dense(const float* X, const float* bx, int64_t n_rows, int64_t ldx, const float* Y, const float* by,
                      int64_t n_other, int64_t ldy, int64_t f, float* D, int64_t ldd, float* dsum, void* stream);
int pinsage_lmf_update(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                       const float* by, int64_t n_other, int64_t ldy, float* X, float* bx, int64_t ldx, int64_t f,
                       const float* D, int64_t ldd, const float* dsum, float* H, int64_t ldh, float* hb,
                       float alpha, float reg, float lr, int* err, void* stream);

/* ------------------------------------------------------------------ node2vec
 * Grover & Leskovec, "node2vec" (2016), as this project defines it: second-order
 * (p, q) walks by rejection sampling on a counter-based generator, and skip-gram
 * with negative sampling fitted on the EXPECTED negatives, a closed objective
 * over the window co-occurrence counts of the walks.  Deterministic; parity with
 * fastnode2vec or gensim is not claimed.
 *
 * pinsage_n2v_walk.  The graph is an undirected CSR: ptr int64 [n_nodes + 1],
 * idx int32 ascending within a row, no duplicates, no self loops; cum int64
 * [nnz] holds per row the inclusive prefix sum of positive integer edge weights
 * (null: unweighted).  walks is int32 [n_walks][length], walk k in row k,
 * position 0 its start starts[k]; positions after the walk's end are -1.  Walk
 * k's generator position is pos = walk_base + k.  Step j >= 1, try t = 0, 1, ..:
 *   (r0, r1, r2, r3) = Philox4x32-10(key = seed, ctr = (j * 256 + t, pos lo, pos hi, offset))
 *   total = the current row's last cum (its degree when unweighted)
 *   pick  = ((r0 | r1 << 32) * total) >> 64
 *   candidate = the first edge of the row whose cum exceeds pick (idx[row start +
 *               pick] when unweighted)
 *   step 1 takes try 0's candidate.  From step 2 on
 *     beta = inv_p if the candidate is the previous node, 1 if it is a neighbour
 *            of the previous node, inv_q otherwise;  M = max(inv_p, 1, inv_q)
 *     accept iff (float)(r2 >> 8) * 0x1p-24f * M < beta
 *   (the first product is exact: one fp32 multiply and one compare); after 256
 *   rejected tries the last candidate is taken.
 * The accepted next node has probability proportional to weight * beta.  With
 * M / min(beta) <= 16 a try is accepted with probability >= 1/16, so the cap of
 * 256 tries distorts at most (15/16)^256 ~ 7e-8 of the steps.  A node without
 * edges ends the walk.  One lane per walk; a walk reads (seed, offset, pos, its
 * start, the graph) only: the result depends neither on the grid nor on how
 * walks are batched into calls.  A start or neighbour id outside [0, n_nodes)
 * sets *err (device, nullable) and is clamped to 0.  Refused (PINSAGE_ERR_ARG,
 * nothing launched, outputs untouched): inv_p or inv_q not finite or not
 * positive; max(inv_p, 1, inv_q) / min(inv_p, 1, inv_q) > 16; length < 1 or
 * >= 2^24; n_nodes < 1 or > INT32_MAX; n_walks < 0 or > INT32_MAX; walk_base < 0;
 * a null ptr or idx; a null starts or walks unless n_walks == 0, which launches
 * nothing.
 *
 * Skip-gram with expected negatives.  C [n, n] is the symmetric CSR of window
 * co-occurrence counts, #(w) = sum_c C_wc, P(c) proportional to #(c)^0.75, tables
 * U (centre) and V (context), s_wc = u_w . v_c, no biases.  The objective to
 * MAXIMISE is
 *   L = sum_wc C_wc log sig(s_wc) + K sum_w #(w) sum_c P(c) log sig(-s_wc)
 *       - (reg / 2)(|U|^2 + |V|^2)
 * One iteration updates every centre row from V, then every context row from
 * the new U; a half-iteration is Jacobi with AdaGrad accumulators from zero.
 * Per row u of X against all of Y, column weight cw, row weight rw, in fp32:
 *   D[u] = sum_all i cw_i sig(x_u . y_i) y_i
 *   g    = sum_obs val_i sig(-(x_u . y_i)) y_i - rw_u D[u] - reg x_u
 *   h   += g^2;   x_u += lr g / sqrt(1e-6 + h)
 * Centre half: X = U, Y = V, cw = P, rw = K #(w).  Context half: X = V, Y = U,
 * cw = K #(w), rw = P(c).  sig as for logistic MF above.
 *
 * pinsage_sgns_dense: D f32 [n_rows][ldd] for every row of X against all of Y f32
 * [n_other][ldy], cw f32 [n_other]: pinsage_lmf_dense's fused kernel with
 * p = cw_i * sig(s) and no row sums.  Exact-f32 MFMA, scores in registers only,
 * items in ascending order, no atomics: the bits of row u depend on x_u, Y and
 * cw only.  Columns [f, ld) are neither read nor written.
 *
 * pinsage_sgns_update: the rest, in place on X and H f32 [n_rows][ldh], from D of
 * the old X; CSR as pinsage_als_half with val f32 > 0, rw f32 [n_rows].  In this
 * order:  s_i = the wave's sum of fma(x.x, y.x, x.y * y.y) (two columns per lane);
 * w_i = val_i * sig(-s_i);  a = fma(w_i, y_i, a) in CSR order from 0;
 * g = fma(-reg, x, fma(-rw_u, D[u], a));  h = fma(g, g, h);
 * x = x + lr * g / sqrt(1e-6 + h).  Row forms as pinsage_lmf_update.  lr == 0
 * leaves X bit for bit and still updates H.  A row without items and with
 * rw_u = 0, reg = 0 keeps x exactly (the step is 0 / sqrt(1e-6 + h)).
 *
 * All pointers are device memory.  err (nullable): as pinsage_als_half.  Refusals
 * (PINSAGE_ERR_ARG, nothing launched, outputs untouched) as the logistic MF
 * pair: f, leading dimensions, alignment, null tables, a null cw, ptr or rw,
 * reg < 0, lr < 0 or either not finite, a count above INT32_MAX, n_other < 1.
 * n_rows == 0 is accepted and launches nothing. */
int pinsage_n2v_walk(const int64_t* ptr, const int32_t* idx, const int64_t* cum, int64_t n_nodes,
                     const int64_t* starts, int64_t n_walks, int64_t length, float inv_p, float inv_q, uint64_t seed,
                     uint32_t offset, int64_t walk_base, int32_t* walks, int* err, void* stream);
int pinsage_sgns_dense(const float* X, int64_t n_rows, int64_t ldx, const float* Y, const float* cw, int64_t n_other,
                       int64_t ldy, int64_t f, float* D, int64_t ldd, void* stream);
int pinsage_sgns_update(const int64_t* ptr, const int32_t* idx, const float* val, const float* rw, int64_t n_rows,
                        const float* Y, int64_t n_other, int64_t ldy, float* X, int64_t ldx, int64_t f, const float* D,
                        int64_t ldd, float* H, int64_t ldh, float reg, float lr, int* err, void* stream);

/* ------------------------------------------------------------------ Bayesian personalised ranking
 * Rendle, Freudenthaler, Gantner, Schmidt-Thieme, "BPR: Bayesian Personalized
 * Ranking from Implicit Feedback" (2009), as this project defines it: the
 * algo="bpr" the reference takes from the implicit package, with the negatives
 * from a counter-based generator and Jacobi AdaGrad half-iterations in place of
 * that package's sampled SGD with racing updates.  Deterministic; parity with
 * that package's numbers is not claimed.
 *
 * Inputs and tables.  R [n_users, n_items] is a CSR whose rows are strictly
 * ascending; only its structure is used, every stored cell is one positive.
 * Tables X [n_users, f], Y [n_items, f] and an item bias b [n_items]; there is
 * no user bias.  Cell e is the e-th stored cell of R; sample t = e * S + s for
 * s < S = negatives.
 *
 * The draw.  For draw round rho, sample t of a cell (u, i), and tries k = 0 .. 15:
 *   (r0, r1, r2, r3) = Philox4x32-10(key = seed, ctr = (rho * 16 + k, t lo, t hi, offset))
 *   j = (uint64(r0) * n_items) >> 32
 *   accept the first j that is not a column of row u   (binary search; j == i is therefore rejected)
 * After 16 rejected tries the sample is void: neg[t] = -1, w[t] = 0.  Otherwise
 * neg[t] = j and, with z = (x_u . y_i + b_i) - (x_u . y_j + b_j), w[t] = sig(-z).
 * The dot is the row plan's: two columns per lane, fmaf(x.x, y.x, x.y * y.y),
 * then the wave sum.  The sigmoid is that of logistic MF above.  neg and w of
 * sample t depend on (seed, rho, offset, t, row u, the tables) only; they do not
 * depend on the grid or on batching.
 *
 * One iteration `it`.  The user half uses draw round 2 it; the item half uses
 * round 2 it + 1 and the new X.  Both halves are Jacobi.
 *   User half, row u, entries in ascending t, for each t (+w_t, y_i) then
 *   (-w_t, y_j).  A void sample contributes (+-0, y_i).
 *   Item half, row i: first the samples whose positive is i, in ascending t,
 *   with (+w_t, x_u); then the non-void samples whose negative is i, in
 *   ascending t, with (-w_t, x_u).
 * Each half then runs, in fp32, per row:
 *   a = 0;  a = fma(val_e, row_e, a) over the entries in that order;   sv = sum of val_e
 *   g = fma(-reg, x, a);  h = fma(g, g, h);  x += lr g / sqrt(1e-6 + h)
 *   item half only:  gb = sv;  hb = fma(gb, gb, hb);  b += lr gb / sqrt(1e-6 + hb)      (bias not regularised, as in LMF)
 * The accumulators start at zero.  For a fixed draw this is ascent on
 * sum_t ln sig(z_t) - (reg/2)(|X|^2 + |Y|^2) over non-void t.
 *
 * pinsage_bpr_sample: neg int32 [nnz negatives] and w f32 [nnz negatives] for
 * every row of the CSR (ptr int64 [n_rows + 1] from 0, idx int32) against X f32
 * [n_rows][ldx], Y f32 [n_other][ldy], by f32 [n_other]; no table is written.
 * The call's cell e is cell cell_base + e of R: a block of rows handed over
 * alone (ptr rebased to 0, its idx, its rows of X, its outputs) draws what it
 * draws in the whole matrix.  One wave per row of at most
 * pinsage_lmf_long_row() cells, the workgroup for a longer one; samples are
 * independent and nothing is reduced.  pinsage_bpr_max_tries() is the 16 above.
 * A positive id outside [0, n_other) sets *err and is clamped to 0.  Refused
 * (PINSAGE_ERR_ARG, nothing launched, outputs untouched): f, leading dimensions
 * and alignment as the logistic MF pair; a null ptr or by; negatives outside
 * [1, 8]; rho outside [0, 2^27); cell_base < 0; a count above INT32_MAX;
 * n_other < 1.  n_rows == 0 is accepted and launches nothing.
 *
 * pinsage_bpr_apply: the signed gathered row sum and the AdaGrad step, in place
 * on X, H f32 [n_rows][ldh] and, unless both are null (the user half), bx and hb
 * f32 [n_rows], for a CSR (ptr, idx int32 in [0, n_other), val f32 of either
 * sign) against Y f32 [n_other][ldy].  sv is summed in CSR order from 0.  Row
 * forms as pinsage_lmf_update: a long row's partial sums of a and sv are added
 * in wave order.  lr == 0 leaves X and bx bit for bit and still updates H and
 * hb.  A row without entries and with reg = 0 keeps x exactly.  err as
 * pinsage_als_half.  Refused: f, leading dimensions, alignment and null tables
 * as the logistic MF pair; a null ptr; exactly one of bx, hb null; reg < 0,
 * lr < 0 or either not finite; a count above INT32_MAX; n_other < 1.
 * n_rows == 0 is accepted and launches nothing. */
int64_t pinsage_bpr_max_tries(void);
int pinsage_bpr_sample(const int64_t* ptr, const int32_t* idx, int64_t n_rows, int64_t cell_base, const float* X,
                       int64_t ldx, const float* Y, const float* by, int64_t n_other, int64_t ldy, int64_t f,
                       int64_t negatives, uint64_t seed, int64_t rho, uint32_t offset, int32_t* neg, float* w, int* err,
                       void* stream);
int pinsage_bpr_apply(const int64_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* Y,
                      int64_t n_other, int64_t ldy, float* X, float* bx, int64_t ldx, int64_t f, float* H, int64_t ldh,
                      float* hb, float reg, float lr, int* err, void* stream);

/* ------------------------------------------------------------------ unsupervised GraphSAGE
 * Hamilton, Ying, Leskovec, "Inductive Representation Learning on Large Graphs"
 * (2017), as this project defines it (csrc/sage.h states the whole model; the
 * reference's GraphSAGE class, baselines.py:517-544, cannot run as written).
 * The graph is an undirected CSR (ptr int64 [n_nodes + 1], idx int32 ascending
 * per row, no duplicates, no self loops) with positive integer weights weight
 * int64 [nnz] (null: unweighted).  All pointers are device memory.
 *
 * pinsage_sage_neighbours: nb int32 [m][fanout], w f32 [m][fanout], row i the
 * neighbour sample (round, nodes[i]).  With deg the length of the node's row v:
 *   deg <= fanout: positions 0 .. deg - 1 in CSR order, the other slots void
 *     (nb = -1, w = 0);
 *   otherwise Floyd's algorithm, for j = 0 .. fanout - 1:
 *     m_j = deg - fanout + j + 1
 *     (r0, r1, r2, r3) = Philox4x32-10(key = seed, ctr = (round * 64 + j, v lo, v hi, offset))
 *     t = ((r0 | r1 << 32) * m_j) >> 64;  c_j = m_j - 1 if t is among c_0 .. c_{j-1}, else t
 *   slot j: nb = idx[row start + c_j], a_j = sqrtf((float)weight) (1 unweighted),
 *   w_j = a_j / (a_0 + a_1 + ...), the sum in slot order from 0 in fp32.
 * The row depends on (seed, offset, round, v, row v) only.  One 32-lane half of
 * a wave per node.  A node id outside [0, n_nodes), or a neighbour id in idx
 * outside it, sets *err (nullable) and is clamped to 0.  Refused
 * (PINSAGE_ERR_ARG, nothing launched, outputs untouched): fanout outside
 * [1, 32]; round outside [0, 2^25); n_nodes outside [1, INT32_MAX]; m < 0 or
 * above INT32_MAX; a null ptr or idx; null nodes, nb or w unless m == 0.
 *
 * pinsage_sage_negatives: neg int32 [B][Q], row i the negatives of anchors[i]
 * = a.  Sample s < Q, tries k = 0 .. 15:
 *   ctr = (round * 16 + k, (a Q + s) lo, hi, offset);  j = (uint64(r0) * n_nodes) >> 32
 *   accept the first j != a that is not in row a (binary search); -1 after 16
 *   rejections.
 * One lane per sample.  An anchor outside [0, n_nodes) sets *err and is clamped
 * to 0.  Refused: Q outside [1, 16]; round outside [0, 2^27); sizes and null
 * pointers as above (B == 0 launches nothing).
 *
 * pinsage_sage_margin_loss: Z f32 [B G][ldz], G = 1 + P + Q, row a G + g the
 * embedding of slot g of anchor group a (slot 0 the anchor, then P positives,
 * then Q negatives); slots int32 [B][G], negative = void.  With
 *   c(a, x) = z_a . z_x / max(sqrt(|z_a|^2 |z_x|^2), 1e-8)
 * c_pos = the smallest cosine over the non-void positives, c_neg = the largest
 * over the non-void negatives (ties: the lowest slot),
 *   loss[a] = max(0, log sig(c_neg) - log sig(c_pos) + margin)
 * for an active anchor (a non-void positive and a non-void negative), else 0;
 * active[a] = 0 / 1; sel int32 [B][2] = the chosen positive and negative slot
 * (index in the group) or -1; dZ f32 [B G][lddz] = *scale (device) times
 * d loss[a] / d Z, every row written (zeros where nothing flows: only the rows
 * a, pos*, neg* of a group can be non-zero).  One wave per group; a lane holds
 * columns 2 lane + 128 c and the next, dots and squared norms are wave sums.
 * sig and softplus as for logistic MF above.  A zero row gives cosine 0 through
 * the clamp, never NaN.  Refused: d outside [4, 512] or d % 4 != 0; ldz or lddz
 * below d or not a multiple of 4; Z or dZ not 16-byte aligned; P outside
 * [1, 64]; Q outside [1, 16]; margin not finite; B < 0; a null pointer unless
 * B == 0.
 *
 * pinsage_sage_lrelu_backward: dp[i][c] = dy[i][c] * (y[i][c] > 0 ? 1 : 0.01)
 * for i < n, c < d: the backward of the GEMM epilogue's leaky ReLU from its
 * output y (dp may be dy).  d % 4 == 0, leading dimensions >= d and multiples
 * of 4, 16-byte aligned pointers. */
int pinsage_sage_neighbours(const int64_t* ptr, const int32_t* idx, const int64_t* weight, int64_t n_nodes,
                            const int64_t* nodes, int64_t m, int64_t fanout, uint64_t seed, int64_t round,
                            uint32_t offset, int32_t* nb, float* w, int* err, void* stream);
int pinsage_sage_negatives(const int64_t* ptr, const int32_t* idx, int64_t n_nodes, const int64_t* anchors, int64_t B,
                           int64_t Q, uint64_t seed, int64_t round, uint32_t offset, int32_t* neg, int* err,
                           void* stream);
int pinsage_sage_margin_loss(const float* Z, int64_t ldz, int64_t d, const int32_t* slots, int64_t B, int64_t P,
                             int64_t Q, float margin, const float* scale, float* loss, int32_t* active, int32_t* sel,
                             float* dZ, int64_t lddz, void* stream);
int pinsage_sage_lrelu_backward(const float* y, int64_t ldy, const float* dy, int64_t lddy, int64_t n, int64_t d,
                                float* dp, int64_t ldp, void* stream);

/* ------------------------------------------------------------------ train-step engine
 * PinSageModel.forward / PinSage.train_batch (pinsage_model.py:246-265,
 * pinsage_training.py:181-214) with device-resident sizes.  Parameters live in
 * one flat fp32 buffer in state_dict order: conv_layers.{i}.Q.weight, Q.bias,
 * W.weight, W.bias (i = 0..n_layers-1), G1.weight, G1.bias, G2.weight; the
 * gradient and Adam buffers use the same layout. */
typedef struct {
  int64_t n_items;  /* feature-table rows (tracks) */
  int64_t d_in;     /* feature dim (dimensions[0]) */
  int64_t hid;      /* hidden_dim (dimensions[1]) */
  int64_t out;      /* out_dim (dimensions[2], <= 128) */
  int64_t n_layers;
  int64_t T;        /* neighbourhood size used by the model */
  int64_t max_pos;  /* max ids per forward (3 * batch_size for a train step) */
} pinsage_engine_config;
typedef struct {
  int64_t ids, pos_rank, z, dz, scalars, n_layers;
  int64_t count_S[8], count_N[8], members_S[8], members_N[8], cap_S[8], cap_N[8], y[8];
  int64_t param_offsets[8];
  int64_t hinge; /* f32 [batch]: cos(q,n) - cos(q,p) + margin of each triple of the last loss */
} pinsage_engine_offsets_t;

int pinsage_engine_create(const pinsage_engine_config* cfg, pinsage_engine** out);
/* Makes no HIP call (safe inside a stream capture, e.g. a finaliser run by the
 * garbage collector while torch.cuda.graph captures): the engine's streams and
 * events are retired to a process-wide pool that later engines reuse. */
void pinsage_engine_destroy(pinsage_engine* e);
/* engines created and not yet destroyed (diagnostics / tests) */
int64_t pinsage_engine_live_count(void);
int64_t pinsage_engine_workspace_bytes(const pinsage_engine* e);
int64_t pinsage_engine_num_params(const pinsage_engine* e);
/* byte offsets of engine outputs inside a workspace (ids int64, pos_rank int32,
 * z/dz f32 [rows][out], scalars f32 {loss, node_feat_loss, sum|h_q|^2, variance}). */
int pinsage_engine_offsets(const pinsage_engine* e, pinsage_engine_offsets_t* out);
/* features f32 [n_items][ld_feats]; tables: nb int32 / normalised weights f32
 * [n_items][ld_table] (first T columns used); grads / adam buffers may be null
 * for inference.
 * Precondition (not checked here: the table is device memory): the first T
 * entries of every row of nb_table are distinct, as the rows of a top-k are.
 * The backward's transposed aggregation sorts each neighbour's (node, weight)
 * pairs by node and relies on that: a node repeated inside one row loses a
 * pair in rows of 17-64 pairs and leaves unwritten row indices in longer ones
 * (see pinsage_agg_transpose).  pinsage_model checks a table once on the host
 * where it is bound (_DeviceTable raises ValueError). */
int pinsage_engine_set_tensors(pinsage_engine* e, const float* feats, int64_t ld_feats,
                               const int32_t* nb_table, const float* w_table, int64_t ld_table,
                               float* params, float* grads, float* adam_m, float* adam_v);
/* on = 0: the engine's next pinsage_engine_frontier calls do not fork its
 * side stream (PINSAGE_CSR_FORK), e.g. while the caller captures them on a
 * branch of a graph (forking off a capture branch, not the capture's origin,
 * sent hipStreamEndCapture into unbounded recursion); 1 (default) restores. */
int pinsage_engine_set_frontier_fork(pinsage_engine* e, int on);
/* Zero the workspace regions the step kernels keep zero after use (loss
 * scatter targets, CSR counters).  Call once per new workspace, before its
 * first forward. */
int pinsage_engine_init_workspace(pinsage_engine* e, void* ws, void* stream);
/* forward of all ids (a train step passes the [B][3] batch flattened); ids must
 * lie in [0, n_items) -- the caller validates them (pinsage_model raises
 * IndexError like the reference's features[nodeset]). */
int pinsage_engine_forward(pinsage_engine* e, void* ws, const int64_t* ids, int64_t n_ids,
                           void* stream);
/* The forward's two phases (pinsage_engine_forward = frontier, then layers).
 * The frontier phase (relevant_nodes_per_layer_precomp, pinsage_model.py:156-168,
 * plus every layer's index tables) reads only the ids and the neighbourhood
 * table -- no parameters -- so a trainer with two workspaces runs the next
 * step's frontier on a side stream while this step's layers and backward run
 * in the other workspace. */
/* pinsage_engine_forward without the backward's plan (the CSR transposes of the
 * neighbour slots): for outputs only (PinSage.embed, evaluation, the first pass
 * of the micro-batched step); no backward may follow on this workspace. */
int pinsage_engine_forward_inference(pinsage_engine* e, void* ws, const int64_t* ids, int64_t n_ids,
                                     void* stream);
int pinsage_engine_frontier(pinsage_engine* e, void* ws, const int64_t* ids, int64_t n_ids,
                            void* stream);
int pinsage_engine_forward_layers(pinsage_engine* e, void* ws, void* stream);
/* Until reset with side_stream = NULL: each pinsage_engine_forward_layers call
 * also runs pinsage_engine_frontier(ws_next, ids_next, n_ids) on side_stream,
 * forked (event) right after the layer-0 Q projection, so it overlaps the rest
 * of the step.  The caller joins side_stream back. */
int pinsage_engine_set_fork(pinsage_engine* e, void* ws_next, const int64_t* ids_next,
                            int64_t n_ids, void* side_stream);
int pinsage_engine_gather_output(pinsage_engine* e, void* ws, int64_t n_ids, float* out,
                                 void* stream);
/* max_margin_loss + monitors on the last forward of a [B][3] batch.  It
 * accumulates the loss cotangent into the workspace's per-row gradient
 * accumulators (the head backward forms dZ from them and re-zeroes them), so a
 * pinsage_engine_backward / _backward_adam MUST follow every loss call on a
 * workspace before its next loss call (an eval-only loss would leave them
 * dirty for the next step).
 * The monitor kernel (loss / node-feature loss / variance scalars, on an engine
 * side stream, dependent on this loss) is enqueued by the next engine call
 * that enqueues work (normally the backward, right behind its first kernel;
 * PINSAGE_DEFER_SIDE=0/1 enqueues it here) and joined at the backward's end.
 * The loss kernels need an out_dim that divides 1024 (4, 8, 16, 32, 64, 128 of
 * the widths pinsage_engine_create accepts: the monitor kernel deals 1024
 * threads over whole rows).  Any other width (12, 96, 100, ...) is refused with
 * PINSAGE_ERR_ARG ("needs an out_dim that divides 1024") before anything is launched;
 * such an engine still serves forwards, pinsage_engine_set_output_grad and
 * the backward. */
int pinsage_engine_loss(pinsage_engine* e, void* ws, int64_t batch_size, float margin,
                        int with_monitors, void* stream);
/* dZ from an upstream gradient of gather_output (single call, autograd path) */
int pinsage_engine_set_output_grad(pinsage_engine* e, void* ws, const float* dout, int64_t n_ids,
                                   void* stream);
/* all parameter gradients from dZ into the grad buffer (overwritten) */
int pinsage_engine_backward(pinsage_engine* e, void* ws, void* stream);
/* Re-arm a workspace whose backward has run for another backward of the same
 * forward (autograd's retain_graph=True: backward(retain_graph=True) then
 * backward again): zeroes the scatter-add targets the backward accumulates
 * into.  The forward's activations and plan are left as they are. */
int pinsage_engine_reset_backward(pinsage_engine* e, void* ws, void* stream);
/* the same backward in two calls, for data-parallel steps that all-reduce the
 * first call's gradients while the second runs (pinsage_training.py:188-191
 * under DP): stage 0 = the head and layers L-1 .. 1 (every gradient but layer
 * 0's is complete in stream order at the call's end), stage 1 = layer 0. */
int pinsage_engine_backward_stage(pinsage_engine* e, void* ws, int stage, void* stream);
/* torch.optim.Adam step over the flat buffers (pinsage_training.py:147,191).
 * coef: device f32[2] = {lr / (1 - beta1^t), sqrt(1 - beta2^t)} for this step
 * t, computed by the caller in double as torch does (kept in device memory so
 * a captured step graph picks up each step's values). */
int pinsage_engine_adam(pinsage_engine* e, const float* coef, double beta1, double beta2, float eps,
                        void* stream);
/* backward followed by that Adam step, scheduled off the critical path: the
 * last gradient (layer 0's Q) applies its own Adam step in the reduction that
 * produces it, and every other parameter is updated beside that reduction.
 * Gradients are still written to the grad buffer; the arithmetic is that of
 * pinsage_engine_backward + pinsage_engine_adam. */
int pinsage_engine_backward_adam(pinsage_engine* e, void* ws, const float* coef, double beta1,
                                 double beta2, float eps, void* stream);

/* Frontier sizes of the last forward in ws (synchronises the stream): S[l] =
 * |S_l| (nodes convolved at layer l), N[l] = |N_l| (distinct neighbours). */
int pinsage_engine_read_counts(const pinsage_engine* e, void* ws, int64_t* S, int64_t* N,
                               void* stream);
/* Expected frontier sizes (e.g. from read_counts): choose GEMM block tiles
 * that fill the chip; sizes stay device-side, hints only affect speed. */
int pinsage_engine_set_hints(pinsage_engine* e, const int64_t* S, const int64_t* N);
/* Layer `layer`'s own neighbourhood table (nb int32 / normalised weights f32,
 * [n_items][ld], first T columns, rows of the layer's nodes used) in place of
 * the engine-wide one from pinsage_engine_set_tensors: the on-the-fly sampler
 * (relevant_nodes_per_layer, pinsage_model.py:142-154) draws every layer's
 * neighbourhoods separately.  nb = wn = null restores the engine-wide table.
 * Read when a frontier is enqueued (pinsage_engine_forward / _frontier).
 * Precondition, as pinsage_engine_set_tensors: the first T entries of every
 * used row of nb are distinct (the sampler's top-k rows are); not checked. */
/* Whether a GEMM site's last launch ran stream-K (1), a whole-K tile (0), or
 * is unknown (-1): the in-context tuner keeps a site's summation order. */
int pinsage_engine_site_stream_k(const pinsage_engine* e, const char* site);
int pinsage_engine_set_layer_table(pinsage_engine* e, int64_t layer, const int32_t* nb,
                                   const float* wn, int64_t ld);
/* The on-the-fly step's virtual nodes (pinsage_fly_sample): ids x0 .. x0 +
 * *n_x - 1 join every frontier's top set, and pinsage_engine_loss hands
 * virtual node j the summed output gradient of its real node xids[j] (call
 * xids[j] / unit), each occurrence's conv output with multiplicity 1
 * (index_put's backward, pinsage_model.py:257-265).  n_x = null: off. */
int pinsage_engine_set_fly(pinsage_engine* e, int64_t x0, const int* n_x, const int64_t* xids, int64_t unit,
                           int64_t x_cap);
/* Per-site GEMM choice (a tuner measures the sites in context and fixes them):
 * site names as the timing sites -- fwd.q_gemm.lN, fwd.w_gemm.lN, bwd.dcat.lN,
 * bwd.dh.lN (block tile config cfg 0..3, stream_k 0/1), bwd.w_wgrad.lN,
 * bwd.q_wgrad.lN, bwd.wgrad.g1, bwd.wgrad.g2 (cfg 0..3 and split-K count
 * splits >= 1).  -1 / 0 leave a field to the launcher's size model; all three
 * unset removes the site's entry.  Speed only: every choice computes the same
 * GEMM (summation order may differ). */
int pinsage_engine_set_gemm_choice(pinsage_engine* e, const char* site, int cfg, int stream_k,
                                   int splits);

/* Per-launch-site HIP-event timing on the launch stream (bench/profiling):
 * enable (also clears), collect after the work (synchronises the events), then
 * read site idx = 0.. until PINSAGE_ERR_ARG: name, total ms, number of calls. */
int pinsage_engine_timing(pinsage_engine* e, int enable);
int pinsage_engine_timing_collect(pinsage_engine* e);
int pinsage_engine_timing_get(const pinsage_engine* e, int idx, char* name, int64_t name_len,
                              double* ms, int64_t* calls);

#ifdef __cplusplus
}
#endif
#endif /* PINSAGE_HIP_H */
