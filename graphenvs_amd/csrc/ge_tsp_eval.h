// Baselines that run as sequential programs, one lane per slot (is_eval_env only).
// TSP-v0: info['heuristic_solution'] = length of a Christofides tour (tsp.py:114-117 calls
// nx.approximation.traveling_salesman_problem: all-pairs Dijkstra, Christofides on the metric closure).  Two launches behind the
// graph kernel, on the slabs it wrote, outside the reset kernels so that the training path (no baseline) carries none of this:
//   ge_k_tsp_closure  one wave per regenerated slot, one LANE per Dijkstra source: integer distances (weight codes = tenths;
//                     spatial: Euclidean lengths in 1/65536) into the slot's scratch block, D[n][n];
//   ge_k_tsp_tour     one LANE per regenerated slot runs ge_christofides.h on that block (spanning tree, exact minimum-weight
//                     perfect matching of the odd nodes by the blossom algorithm, Eulerian circuit, shortcutting) and replaces the
//                     double-tree value 2 x MST the graph kernel left in heuristic[].
// This is an evaluation-time path (the reference spends seconds per reset in networkx here): lanes run unrelated sequential
// programs, nothing is tuned beyond keeping every slot of a launch busy side by side.
#pragma once
#include "ge_params.h"
#include "ge_reset.h"

#ifdef GE_EMU
#define GE_CH_FN static inline
#define GE_CR_FN static inline
#else
#define GE_CH_FN static __device__
#define GE_CH_HD static __host__ __device__ inline
#define GE_CR_FN static __device__
#define GE_CR_HD static __host__ __device__ inline
#endif
#include "ge_christofides.h"
#include "ge_clique_removal.h"
#include "ge_kou_exact.h"

#define GE_TSP_EVAL_THREADS 64

GE_DEV int32_t ge_tsp_units(const GeParams &P, double w) { return (int32_t)llrint(w * 65536.0); }

// items of the launch: every slot (full reset) or the queued ones; `pre` (LDS) holds the queue prefix in queue mode
GE_DEV int ge_tsp_count(const GeParams &P, int *pre, int queue) {
  if (!queue) return P.B;
  if (ge_tid() < GE_WAVE) ge_queue_prefix_wave(P, pre, ge_tid());
  ge_sync();
  return pre[(P.B + GE_STEP_BLOCK - 1) / GE_STEP_BLOCK];
}

GE_HOSTDEV uint64_t ge_steiner_slot_bytes(int n, int m, int T) {
  return ((((uint64_t)(2 * m + 1) * 2) + 15) & ~15ull) + ((((uint64_t)(2 * m + 1) * 8) + 15) & ~15ull) + ge_kou_arena_bytes(n, m, T);
}

// per-slot work space of the sequential is_eval_env baselines; 0 = none
GE_HOSTDEV uint64_t eval_slot_bytes(const GeParams &P) {
  if (!P.is_eval) return 0;
  if (P.env_type == GE_TSP) return ge_ch_slot_bytes(P.n);
  if (P.env_type == GE_MAX_INDEPENDENT_SET && !P.weighted) return ge_cr_slot_bytes(P.n, P.m);
  if (P.env_type == GE_STEINER_TREE && P.n_dests > 1 && P.n_dests < P.n - 1) return ge_steiner_slot_bytes(P.n, P.m, P.T);  // steiner_tree.py:78-87: the Kou branch
  return 0;
}

// RAGGED (multi-class engine): PG is the engine-wide block (all slots, the queue) and item `env` is a global slot; the baseline runs
// on its class's slabs (local slot), its class's eval_scratch and per-slot size.  Returns false for a class without this baseline
// (SteinerTree: n_dests outside the Kou branch).  Uniform engine: the launch's own block, scratch and size.
template <bool RAGGED>
GE_DEV bool ge_eval_item(const GeParams &PG, const GeRagged &R, int env, uint8_t *scratch, uint64_t slot_bytes, const GeParams *&P,
                         int &local, uint8_t *&blk) {
  if constexpr (RAGGED) {
    const int cls = R.slot_class[env];
    P = &R.classes[cls];
    local = env - R.class_start[cls];
    const uint64_t sb = eval_slot_bytes(*P);
    blk = (uint8_t *)P->buf.eval_scratch + (uint64_t)local * sb;
    return sb != 0;
  } else {
    (void)R;
    P = &PG; local = env; blk = scratch + (uint64_t)env * slot_bytes;
    return true;
  }
}

template <bool RAGGED>
GE_KERNEL ge_k_tsp_closure(GeParams PG, GeRagged R, int queue, uint8_t *scratch, uint64_t slot_bytes, int pre_off) {
  uint64_t *done_all = (uint64_t *)ge_dyn_smem();  // [64 lanes][W] settled sets (W: the widest class's)
  int *pre = (int *)(ge_dyn_smem() + pre_off);
  const int count = ge_tsp_count(PG, pre, queue);
  const int lane = ge_tid();
  uint64_t *done = done_all + lane * PG.W;
  for (int q = ge_bid(); q < count; q += ge_gdim()) {
    const int genv = queue ? ge_queue_slot(PG, pre, q) : q;
    const GeParams *Pp; int env; uint8_t *blk;
    if (!ge_eval_item<RAGGED>(PG, R, genv, scratch, slot_bytes, Pp, env, blk)) continue;
    const GeParams &P = *Pp;
    const int n = P.n, W = P.W;
    const ge_buffers &G = P.buf;
    int32_t *D = (int32_t *)blk;
    const int32_t *rp = G.row_ptr + (int64_t)env * (n + 1);
    const int64_t ebase = (int64_t)env * P.E;
    for (int s = lane; s < n; s += GE_WAVE) {  // array Dijkstra from s: the row D[s][*] is the tentative-distance array
      int32_t *row = D + (int64_t)s * n;
      for (int v = 0; v < n; v++) row[v] = INT32_MAX;
      for (int w = 0; w < W; w++) done[w] = 0ull;
      row[s] = 0;
      for (int it = 0; it < n; it++) {
        int v = -1; int32_t best = INT32_MAX;
        for (int u = 0; u < n; u++) { const int32_t d = row[u]; if (d < best && !((done[u >> 6] >> (u & 63)) & 1ull)) { best = d; v = u; } }
        if (v < 0) break;
        done[v >> 6] |= 1ull << (v & 63);
        if (P.spatial) {  // sw64: float64 lengths in ascending-neighbour order
          int j = rp[v];
          for (int w = 0; w < W; w++)
            for (uint64_t bits = G.adj_bits[((int64_t)env * n + v) * W + w]; bits; bits &= bits - 1, j++) {
              const int u = w * 64 + ge_ctz64(bits); const int32_t d = best + ge_tsp_units(P, G.sw64[ebase + j]);
              if (d < row[u]) row[u] = d;
            }
        } else {
          for (int k = rp[v]; k < rp[v + 1]; k++) {
            const uint16_t cw = G.colw[ebase + k]; const int u = cw >> 4; const int32_t d = best + (int32_t)(cw & 15);
            if (d < row[u]) row[u] = d;
          }
        }
      }
    }
  }
}

template <bool RAGGED>
GE_KERNEL ge_k_tsp_tour(GeParams PG, GeRagged R, int queue, uint8_t *scratch, uint64_t slot_bytes) {
  int *pre = (int *)ge_dyn_smem();
  const int count = ge_tsp_count(PG, pre, queue);
  for (int q = ge_bid() * GE_TSP_EVAL_THREADS + ge_tid(); q < count; q += ge_gdim() * GE_TSP_EVAL_THREADS) {
    const int genv = queue ? ge_queue_slot(PG, pre, q) : q;
    const GeParams *Pp; int env; uint8_t *blk;
    if (!ge_eval_item<RAGGED>(PG, R, genv, scratch, slot_bytes, Pp, env, blk)) continue;
    const GeParams &P = *Pp;
    const int n = P.n;
    ge_ch c;
    c.err = 0;
    ge_ch_carve(&c, blk + ge_ch_align((uint64_t)n * (uint64_t)n * 4u), n);
    c.D = (const int32_t *)blk;
    const int64_t tot = ge_christofides_tour(&c);
    if (tot >= 0) P.buf.heuristic[env] = (double)tot / (P.spatial ? 65536.0 : 10.0);  // else: the double-tree walk stays
  }
}

// MaxIndependentSet-v0 baseline (is_eval_env, unweighted): len(nx.approximation.maximum_independent_set(G))
// (max_independent_set.py:63-67), networkx's clique removal reproduced exactly (ge_clique_removal.h: dict orders of the graph
// copies, CPython's set tables).  One LANE per regenerated slot on the slot's scratch block; replaces the min-degree greedy value
// the graph kernel left in heuristic[] (which stays if the work space were ever too small).  Evaluation-time path, like the above.
template <bool RAGGED>
GE_KERNEL ge_k_mis_baseline(GeParams PG, GeRagged R, int queue, uint8_t *scratch, uint64_t slot_bytes) {
  int *pre = (int *)ge_dyn_smem();
  const int count = ge_tsp_count(PG, pre, queue);
  for (int q = ge_bid() * GE_TSP_EVAL_THREADS + ge_tid(); q < count; q += ge_gdim() * GE_TSP_EVAL_THREADS) {
    const int genv = queue ? ge_queue_slot(PG, pre, q) : q;
    const GeParams *Pp; int env; uint8_t *blk;
    if (!ge_eval_item<RAGGED>(PG, R, genv, scratch, slot_bytes, Pp, env, blk)) continue;
    const GeParams &P = *Pp;
    const int n = P.n;
    const ge_buffers &G = P.buf;
    ge_cr_work w;
    ge_cr_carve(&w, blk, n, P.m);
    const int32_t *rp = G.row_ptr + (int64_t)env * (n + 1);
    const int64_t ebase = (int64_t)env * P.E;
    for (int v = 0; v <= n; v++) w.ga.off[v] = rp[v];
    for (int k = 0; k < P.E; k++) w.ga.adj[k] = (uint16_t)(G.colw[ebase + k] >> 4);  // insertion-order columns
    const int32_t r = ge_cr_solve(&w);
    if (r >= 0) G.heuristic[env] = (double)r;
  }
}

// SteinerTree-v0 baseline (is_eval_env, 1 < n_dests < n - 1): the sum of delays over networkx's Kou Steiner tree
// (steiner_tree.py:84-87), reproduced exactly (ge_kou_exact.h: heap-ordered Dijkstra paths, stable Kruskal order over subgraph
// views, CPython's set tables for tuples and ints, float64 sum order).  One LANE per regenerated slot; replaces the own Kou-style
// value the graph kernel left in heuristic[] (which stays if the work space were ever too small).

template <bool RAGGED>
GE_KERNEL ge_k_steiner_baseline(GeParams PG, GeRagged R, int queue, uint8_t *scratch, uint64_t slot_bytes) {
  int *pre = (int *)ge_dyn_smem();
  const int count = ge_tsp_count(PG, pre, queue);
  for (int q = ge_bid() * GE_TSP_EVAL_THREADS + ge_tid(); q < count; q += ge_gdim() * GE_TSP_EVAL_THREADS) {
    const int genv = queue ? ge_queue_slot(PG, pre, q) : q;
    const GeParams *Pp; int env; uint8_t *blk;
    if (!ge_eval_item<RAGGED>(PG, R, genv, scratch, slot_bytes, Pp, env, blk)) continue;
    const GeParams &P = *Pp;
    const int n = P.n;
    const ge_buffers &G = P.buf;
    uint16_t *adj = (uint16_t *)blk;
    double *w = (double *)(blk + ((((uint64_t)(2 * P.m + 1) * 2) + 15) & ~15ull));
    const int64_t ebase = (int64_t)env * P.E;
    for (int k = 0; k < P.E; k++) { const uint16_t cw = G.colw[ebase + k]; adj[k] = (uint16_t)(cw >> 4); w[k] = ge_wlut(cw & 15); }
    ge_cr_arena a;
    a.base = (uint8_t *)w + ((((uint64_t)(2 * P.m + 1) * 8) + 15) & ~15ull); a.top = 0; a.peak = 0; a.cap = ge_kou_arena_bytes(n, P.m, P.T); a.err = 0;
    ge_kou_in g;
    g.n = n; g.m = P.m; g.T = P.T; g.off = G.row_ptr + (int64_t)env * (n + 1); g.adj = adj; g.w = w; g.terms = G.terminals + (int64_t)env * P.T;
    int err = 0;
    const double v = ge_kou_exact(&g, &a, &err);
    if (!err) G.heuristic[env] = v;
  }
}
