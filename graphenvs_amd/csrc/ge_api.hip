// C ABI of libgraphenvs_hip.so (include/graphenvs.h): config validation, buffer binding and
// kernel launches.  No device allocation, no synchronisation (except ge_timed_rollout).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <memory>
#include <new>
#include <vector>

#include "ge_params.h"
#include "ge_platform.h"
#include "ge_reset.h"
#include "ge_features.h"
#include "ge_step.h"
#include "ge_tsp_eval.h"
#include "ge_spare.h"
#include "ge_policy.h"

// An engine's launch geometry: filled once when the engine is created (finish_create), read by every launch, computed nowhere else.
// The size classes of a multi-class engine are grouped into LDS buckets (by n_nodes: <= 128, <= 256, <= 512, larger), and the graph
// kernel and the generic feature kernel are launched once per bucket with the dynamic LDS -- hence the residency -- of the bucket's
// largest class (round 2 ran every class at the occupancy of n = 512: one workgroup per CU).  A uniform engine is ONE bucket whose
// only class is e->P; its launches pass the bucket index -1 (no class filter in the kernels).
#define GE_MAX_BUCKETS 4
struct GeBucket {
  bool used;
  bool list_only;  // classes on the n <= 64 fast path only: the generic feature kernel serves that path's fallback list (slots too deep for it)
  struct { int lds, pre, grid; } graph;             // graph kernel: dynamic LDS bytes, GeLds.pre of the launch, resident workgroups
  struct { int lds, pre_off, threads, grid; } gen;  // generic feature kernel (list_only: grid is the whole launch)
};
struct GePlan {
  int n_buckets;  // 1: uniform engine
  GeBucket bk[GE_MAX_BUCKETS];
  int nseed;      // seeding workgroups at the head of the queue-mode reset launch (64 queued slots each)
  int nseed2;     // split seeding (GE_SEED_SPLIT; a uniform engine on the n <= 64 fast path, until spares are attached): pass-2 workgroups
                  // at the head of ge_k_features64's queue launch, GE_SEED2_ITEMS queued slots each; 0: the graph launch seeds to the end
  bool feat_fast;                       // a class takes the n <= 64 feature kernel (spatial TSP: float64 weights do not fit its LDS)
  int f64_lds, f64_pre_off, feat_grid;  // that kernel's launch; feat_grid without it: resident workgroups of the generic kernel at the largest class's carve
  GeLds inject;   // ge_inject_state runs the graph kernel on this carve (inject_carve)
  int pol_group, pol_grid;  // policy head (ge_policy.h): lanes per row -- the power of two covering the widest mask row, 64 above 32 actions -- and workgroups
};
static int bucket_of(int n) { return n <= 128 ? 0 : (n <= 256 ? 1 : (n <= 512 ? 2 : 3)); }
static bool takes_generic(const GeParams &C) { return C.n > 64 || C.spatial; }  // the class's slots run the generic feature kernel, not the fast path

// The kernel instantiations an engine runs, chosen once when it is created (select_kernels).  Every launch and every raise of a
// dynamic-LDS limit takes its kernel from here, so the instantiation whose limit was raised is the one that is launched.
typedef void (*GeBaselineFn)(GeParams, GeRagged, int, uint8_t *, uint64_t);
struct GeKernels {
  void (*reset)(GeParams, GeRagged, const uint32_t *, GeRun, GeInject, int, int);
  void (*features)(GeParams, GeRagged, GeRun, int, int);
  void (*features64)(GeParams, GeRagged, GeRun, int);
  void (*feat_combine)(GeParams, GeRagged, GeRun);
  void (*swap)(GeParams, GeRagged, GeRagged, ge_buffers, int);
  void (*sample)(GeParams, GeRagged, uint64_t, int64_t *);
  // [GE_LOGITS_F32 / GE_LOGITS_BF16 / GE_LOGITS_F16: the logits' storage type][GE_POL_SAMPLE / GE_POL_GREEDY / GE_POL_EVALUATE]
  void (*policy_head[GE_LOGITS_DTYPES][GE_POL_MODES])(GeParams, GeRagged, GePolicyIO);
  void (*policy_grad[GE_LOGITS_DTYPES])(GeParams, GeRagged, GePolicyIO);  // the logits gradient of GE_POL_EVALUATE's outputs
  void (*dc_range)(GeParams, GeRagged, const int64_t *);
  void (*tsp_closure)(GeParams, GeRagged, int, uint8_t *, uint64_t, int);
  GeBaselineFn tsp_tour, mis_baseline, steiner_baseline;
  void (*step[2])(GeParams, GeRagged, const int64_t *, uint64_t);  // [SAMPLE]
  int step_threads;
  size_t step_lds;
  bool step_quad;  // step[] is the quad-per-slot kernel of the edge-action envs (ge_k_step_edge)
  void (*step_path64[2][2])(GeParams, const int64_t *, uint64_t);  // [SAMPLE][SPARES], set where it takes the place of step[] (path64)
};

struct ge_engine {
  GeParams P;
  ge_config cfg;
  GeKernels k = {};
  GePlan plan = {};
  hipEvent_t ev[4];
  bool have_events = false;
  // multi-class ("ragged") engine: P is then the engine-wide block (B = all slots, global queue / seed / episode / mt_state arrays,
  // n / m / W = the widest class) and R names the device copy of the class table
  int n_classes = 0;
  GeRagged R = {};
  int aw_max;     // the widest mask row (multi-class engine: over the classes; edge-action envs: 2 m words, not a function of n)
  std::vector<GeParams> classes;  // host copy (ge_vectorize launches per class)
  bool loaded = false;    // the slots hold an episode (ge_reset or ge_inject_state ran)
  bool seeded = false;    // the generator-state ring is valid (ge_reset, or ge_inject_state with seeds)
  bool streams = false;   // stream_state holds the streams a regeneration left behind (ge_reset; a restored snapshot)
  // episode prefetch (ge_attach_spares): PS is the engine seen through its spare image -- the same geometry, generator ring,
  // seed[] / episode[] and work lists, but every per-slot slab is the image's and the queue is the refill list
  bool spares = false;
  GeParams PS;
  GeRagged RS = {};                // multi-class engine: class table whose bufs are the images
  std::vector<GeParams> classesS;  // its host copy
  int period = 0, swap_parts = 1;
  int64_t pending_calls = 0;       // ge_reset_pending calls since the last refill
  int32_t *refill_list = nullptr, *refill_count = nullptr;
};

// ---- what a reset-path launch does (GeRun, ge_params.h): the only places where a request becomes flags
static GeRun run_full() { GeRun r = {GE_ITEMS_ALL, 1, 0, 0, 0, 0, 0}; return r; }                         // ge_reset
static GeRun run_inject(bool seeds) { GeRun r = {GE_ITEMS_ALL, seeds ? 2 : 0, 0, 0, 1, 0, 0}; return r; }  // ge_inject_state
static GeRun run_continue() { GeRun r = {GE_ITEMS_ALL, 0, 1, 1, 0, 0, 0}; return r; }                     // ge_reset_continue
// finished slots regenerated in place.  Without spares the launch that moves a slot to episode e + 1 refills ring entry e with
// episode e + GE_SEED_DEPTH; with spares every regeneration of a slot -- refill or in place -- seeds the episode after the one it
// generates, two past the one seed[] / episode[] name
static GeRun run_queue(const ge_engine *e) { GeRun r = {GE_ITEMS_QUEUE, 0, 1, 0, 0, 0, e->spares ? 2 : GE_SEED_DEPTH, e->plan.nseed2}; return r; }
static GeRun run_refill() { GeRun r = {GE_ITEMS_QUEUE, 0, 1, 0, 0, 1, 2}; return r; }
static GeRun as_list(GeRun r) { r.items = GE_ITEMS_LIST; return r; }  // the feature kernels' fallback list of the same launch sequence


static thread_local char g_err[256] = "";
static int fail(int code, const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); return code; }
extern "C" const char *ge_last_error(void) { return g_err; }
extern "C" int ge_abi_version(void) { return GE_ABI_VERSION; }
#ifndef GE_SOURCE_HASH
#define GE_SOURCE_HASH "unknown"
#endif
static const char g_source_hash[] = "GE_SOURCE_HASH=" GE_SOURCE_HASH;  // the marker lets the host read the hash from the file's bytes
extern "C" const char *ge_source_hash(void) { return g_source_hash + 15; }

static const int kMaxLds = 160 * 1024;
static const GeInject kNoInject = {nullptr, nullptr, nullptr, nullptr, nullptr};
static int step_blocks(int64_t B) { return (int)((B + GE_STEP_BLOCK - 1) / GE_STEP_BLOCK); }  // workgroups of GE_STEP_BLOCK slots (one queue counter each)
// LDS bytes of the queue prefix of an engine of B slots: the kernels index it with step_blocks(B) + 2 entries
static int prefix_bytes(int64_t B) { return (step_blocks(B) + 2) * 4; }
// every dynamic-LDS size an engine would launch with fits a CU
static bool carves_fit(std::initializer_list<int> bytes) { for (int b : bytes) if (b > kMaxLds) return false; return true; }
// workgroups that stay resident at `lds` bytes each (256 CUs, at most 16 per CU), no more than one per slot
static int resident_grid(int lds, int64_t B) {
  int per_cu = kMaxLds / (lds > 0 ? lds : 1);
  if (per_cu > 16) per_cu = 16;
  if (per_cu < 1) per_cu = 1;
  return 256 * per_cu > B ? (int)B : 256 * per_cu;
}
static int64_t obs_len(const GeParams &P) { return (int64_t)P.n * P.F + (int64_t)P.E * P.Fe + 2 * (int64_t)P.E; }  // flat observation of one slot
// parenting >= 2 of LongestPath / TSP: the step kernel carries the residual-graph walks (PRUNE 1: node sets of up to GE_MAXW words
// in registers; PRUNE 2: in prune_scratch)
static bool prunes(const GeParams &P) { return (P.env_type == GE_LONGEST_PATH || P.env_type == GE_TSP) && P.parenting >= 2; }
#ifndef GE_NP_EARLY_MAX
#define GE_NP_EARLY_MAX 256  // graphs up to this size hold the n x n delay matrix in LDS (a test build lowers it to run the late path, ge_np_draws_edges, on small graphs)
#endif

// the reset kernel is instantiated per env type (ge_k_reset<ENV>): run `stmt` with ENV bound to the runtime env type
#define GE_FOR_ENV(env_type, stmt)                                                           \
  do {                                                                                       \
    switch (env_type) {                                                                      \
      case GE_SHORTEST_PATH: { constexpr int ENV = GE_SHORTEST_PATH; stmt; break; }            \
      case GE_LONGEST_PATH: { constexpr int ENV = GE_LONGEST_PATH; stmt; break; }              \
      case GE_STEINER_TREE: { constexpr int ENV = GE_STEINER_TREE; stmt; break; }              \
      case GE_TSP: { constexpr int ENV = GE_TSP; stmt; break; }                                \
      case GE_DENSEST_SUBGRAPH: { constexpr int ENV = GE_DENSEST_SUBGRAPH; stmt; break; }      \
      case GE_MAX_INDEPENDENT_SET: { constexpr int ENV = GE_MAX_INDEPENDENT_SET; stmt; break; } \
      case GE_MULTICAST_ROUTING: { constexpr int ENV = GE_MULTICAST_ROUTING; stmt; break; }    \
      case GE_DISTRIBUTION_CENTER: { constexpr int ENV = GE_DISTRIBUTION_CENTER; stmt; break; } \
      default: { constexpr int ENV = GE_PERISHABLE_DELIVERY; stmt; break; }                    \
    }                                                                                        \
  } while (0)

// GeParams.nocolw engines: ge_inject_state runs the graph kernel on the full LDS carve (the injected rows need the {neighbour, code}
// list the reset of such an engine does without)
static GeLds inject_carve(const GeParams &P, int queue_B) {
  if (!P.nocolw) return P.lds;
  GeParams Pi = P; Pi.nocolw = 0; Pi.nowsort = 0; ge_make_lds(Pi, queue_B);
  return Pi.lds;
}

static int derive(const ge_config *cfg, GeParams &P, int queue_B = 0) {
  if (!cfg) return fail(GE_E_BADARG, "null config");
  memset(&P, 0, sizeof(P));
  const int t = cfg->env_type, n = cfg->n_nodes, m = cfg->n_edges;
  if (t < GE_SHORTEST_PATH || t > GE_PERISHABLE_DELIVERY) return fail(GE_E_BADARG, "unknown env_type");
  if (cfg->num_envs < 1) return fail(GE_E_BADARG, "num_envs must be >= 1");
  if (n < 3 || n > 4095) return fail(GE_E_BADARG, "n_nodes must be in [3, 4095]");
  const int ng = (t == GE_DENSEST_SUBGRAPH) ? n - 1 : n;  // densest_subgraph.py:59
  const double max_edges = (double)ng * (ng - 1) / 2.0;
  if (m < ng - 1) return fail(GE_E_BADARG, "n_edges < nodes-1: no connected graph exists (the reference would loop forever)");
  if (m > max_edges) return fail(GE_E_BADARG, "n_edges exceeds the complete graph");
  // G(n, m) is sampled by rejection until it is connected.  P(connected) ~ exp(-n e^(-2m/n)) (Erdos-Renyi): below 1e-7 the
  // reference would spin for hours per reset and a device loop of that length is a hung GPU -- refuse it loudly instead.
  if (m < max_edges && (double)ng * exp(-2.0 * (double)m / (double)ng) > 16.2)
    return fail(GE_E_UNSUPPORTED, "n_edges is so small for n_nodes that a random G(n, m) is connected with probability < 1e-7: the reference's rejection loop would not terminate in practice");
  // TSP also rejects graphs with a node of degree 1 (tsp.py:65-68): P(none) ~ exp(-n d e^(-d)) with d = 2m/n
  if (t == GE_TSP && m < max_edges && (double)n * (2.0 * m / n) * exp(-2.0 * (double)m / (double)n) > 16.2)
    return fail(GE_E_UNSUPPORTED, "n_edges is so small for n_nodes that a random G(n, m) has no degree-1 node with probability < 1e-7: the TSP rejection loop would not terminate in practice");
  // constructor asserts of the reference
  if (t == GE_SHORTEST_PATH && cfg->parenting != -1) return fail(GE_E_BADARG, "Parenting is not available for shortest path (shortest_path.py:26)");
  if (t == GE_STEINER_TREE && cfg->parenting != -1) return fail(GE_E_BADARG, "Parenting not available for this environment (steiner_tree.py:29)");
  if (t == GE_LONGEST_PATH && (cfg->parenting < 0 || cfg->parenting > 3)) return fail(GE_E_BADARG, "parenting must be in [0,1,2,3] (longest_path.py:29)");
  if (t == GE_TSP && cfg->parenting != 1 && cfg->parenting != 2) return fail(GE_E_BADARG, "Parenting must be either 1 or 2 (tsp.py:25)");
  if (t == GE_DENSEST_SUBGRAPH && cfg->parenting != 0 && cfg->parenting != 1) return fail(GE_E_BADARG, "Parenting must be 0 or 1 (densest_subgraph.py:28)");
  if (t == GE_DENSEST_SUBGRAPH && cfg->weighted) return fail(GE_E_BADARG, "Weighted graphs not supported for this env (densest_subgraph.py:29)");
  if (t == GE_TSP && cfg->spatial && !cfg->weighted) return fail(GE_E_BADARG, "Spatial TSP must be weighted (tsp.py:27)");
  if ((t == GE_STEINER_TREE || t == GE_MULTICAST_ROUTING) && (cfg->n_dests < 1 || cfg->n_dests > n - 1)) return fail(GE_E_BADARG, "n_dests must be in [1, n_nodes-1]");
  if (t == GE_PERISHABLE_DELIVERY && cfg->parenting != 1) return fail(GE_E_BADARG, "Parenting must be 1! (perishable_product_delivery.py:30)");
  if (t == GE_PERISHABLE_DELIVERY && (cfg->n_dests < 1 || cfg->n_dests > 5)) return fail(GE_E_BADARG, "Max 5 products! (perishable_product_delivery.py:35)");
  if (t == GE_PERISHABLE_DELIVERY && 2 * cfg->n_dests > n) return fail(GE_E_BADARG, "2 * n_products exceeds n_nodes: the reference would loop forever");
  if (t == GE_PERISHABLE_DELIVERY && !(cfg->dt_max >= cfg->dt_min && cfg->dt_min > 0.0)) return fail(GE_E_BADARG, "dt_min / dt_max must be the constructor's delivery-time window (0 < dt_min <= dt_max)");
  if (t == GE_DISTRIBUTION_CENTER && cfg->parenting != 1 && cfg->parenting != 2) return fail(GE_E_BADARG, "parenting must be 1 or 2 (distribution_center.py:32)");
  if (t == GE_DISTRIBUTION_CENTER && (cfg->n_dests < 0 || cfg->n_dests > n)) return fail(GE_E_BADARG, "target_count must be in [0, n_nodes]");
  if (t == GE_DISTRIBUTION_CENTER && !(cfg->max_distance >= 0.0)) return fail(GE_E_BADARG, "max_distance must be >= 0");
  if (t == GE_MULTICAST_ROUTING && (cfg->parenting < 1 || cfg->parenting > 4)) return fail(GE_E_BADARG, "Invalid parenting type (multicast_routing.py:34-35)");

  P.env_type = t; P.B = cfg->num_envs; P.n = n; P.m = m; P.E = 2 * m; P.W = (n + 63) / 64; P.ng = ng;
  const bool edge_env = (t == GE_STEINER_TREE || t == GE_MULTICAST_ROUTING);
  P.nflag = (t == GE_TSP || t == GE_MULTICAST_ROUTING) ? 4 : (t == GE_DENSEST_SUBGRAPH ? 1 : (t == GE_DISTRIBUTION_CENTER ? 5 : (t == GE_PERISHABLE_DELIVERY ? 16 : 2)));  // utils.py:32-73
  P.F = P.nflag + 5;
  P.Fe = edge_env ? 2 : 1;
  P.A = edge_env ? P.E : n;  // steiner_tree.py:117, multicast_routing.py:155-157
  P.AW = (P.A + 63) / 64;
  P.T = edge_env ? (cfg->n_dests + 1 > 2 ? cfg->n_dests + 1 : 2) : 2;
  if (t == GE_DISTRIBUTION_CENTER) { P.T = cfg->n_dests > 2 ? cfg->n_dests : 2; P.max_distance = cfg->max_distance; }
  if (t == GE_PERISHABLE_DELIVERY) { P.T = 2 * cfg->n_dests; P.dt_min = cfg->dt_min; P.dt_max = cfg->dt_max; }
  P.weighted = cfg->weighted ? 1 : 0; P.parenting = cfg->parenting; P.n_dests = cfg->n_dests;
  P.spatial = (t == GE_TSP && cfg->spatial) ? 1 : 0;
  P.is_eval = cfg->is_eval_env ? 1 : 0; P.autoreset = cfg->autoreset == 2 ? 2 : (cfg->autoreset ? 1 : 0);
  P.complete = (m >= max_edges) ? 1 : 0;
  P.div_m = ((1ull << 40) / (uint64_t)(ng > 1 ? ng - 1 : 1)) + 1ull;
  P.n_choices = (cfg->n_choices < 0) ? floor((double)n / exp(1.0)) : cfg->n_choices;  // densest_subgraph.py:38-39
  P.env_index_base = cfg->env_index_base; P.seed_stride = cfg->seed_stride;
  P.node_id_base = cfg->node_id_base;
  P.edge_row_stride = cfg->edge_row_stride > 0 ? cfg->edge_row_stride : (int64_t)cfg->num_envs * 2 * m;
  P.np_early = (t == GE_TSP || t == GE_MAX_INDEPENDENT_SET || t == GE_DENSEST_SUBGRAPH || !cfg->weighted || n <= GE_NP_EARLY_MAX) ? 1 : 0;  // nibble matrix of n*n/2 bytes <= 32 KiB
  // few slots regenerate per step when graphs are large (long episodes): 8 workgroups share a slot's sources.  The number of
  // parts fixes the order in which a node's float64 betweenness is added up, so it depends on the geometry only, not on the
  // batch size (a shard of a batch must reproduce the unsharded run bit for bit); only a partial-sum scratch beyond 16 GiB
  // halves it
  P.feat_parts = 1;
  if (n > 64) { int parts = 8; while (parts > 1 && (int64_t)cfg->num_envs * parts * n * 8 > (16ll << 30)) parts >>= 1; P.feat_parts = parts; }
  if (P.complete && ng == n) P.feat_parts = 1;  // no BFS sources to share: betweenness and closeness of a complete graph are constants
  if (!P.complete && m > 65535) return fail(GE_E_TOOBIG, "n_edges > 65535 for a non-complete graph");
  if (P.E > (1 << 24)) return fail(GE_E_TOOBIG, "too many edges");
  if (cfg->num_envs > 8192 * GE_STEP_BLOCK) return fail(GE_E_TOOBIG, "num_envs > 2M per engine");
  P.nocolw = (t == GE_TSP && P.complete && ng == n && !P.is_eval && !P.spatial && !getenv("GE_KEEP_COLW")) ? 1 : 0;
  P.nowsort = (P.nocolw && n > 64) ? 1 : 0;
  const int qB = queue_B > 0 ? queue_B : P.B;
  ge_make_lds(P, qB);
  ge_make_ldsf(P, qB);
  ge_tune_feat_parts(P);
  // every carve finish_create launches with, so that the layout query refuses what ge_create / ge_create_ragged would: the graph
  // kernel's (ge_inject_state included), and the two a multi-class engine lengthens by a second queue prefix behind its widest class
  const int pre2 = prefix_bytes(qB);
  if (!carves_fit({P.lds.total + (P.lds.pre != 0 ? pre2 : 0), inject_carve(P, qB).total, P.ldsf.total + pre2}))
    return fail(GE_E_TOOBIG, "per-env graph does not fit 160 KiB of LDS");
  return GE_OK;
}

extern "C" int ge_get_layout(const ge_config *cfg, ge_layout *out) {
  GeParams P;
  int rc = derive(cfg, P);
  if (rc != GE_OK) return rc;
  if (!out) return fail(GE_E_BADARG, "null layout");
  out->F = P.F; out->Fe = P.Fe; out->A = P.A; out->W = P.W; out->E = P.E;
  out->total_nodes = (int64_t)P.B * P.n; out->total_edges = (int64_t)P.B * P.E;
  out->obs_len = obs_len(P);
  out->reset_lds_bytes = P.lds.total;
  out->feat_parts = P.feat_parts;
  out->eval_scratch_bytes = (int64_t)((uint64_t)P.B * eval_slot_bytes(P));
  out->prune_scratch_words = (prunes(P) && P.W > GE_MAXW) ? (int64_t)P.B * 4 * P.W : 0;
  return GE_OK;
}

extern "C" int ge_destroy(ge_engine *e);

static int check_buffers(const GeParams &P, const ge_buffers *bufs) {
  const void *need[] = {bufs->x, bufs->edge_index, bufs->edge_attr, bufs->row_ptr, bufs->colw, bufs->scode, bufs->adj_bits, bufs->slot_rec,
                        bufs->terminals, bufs->node_bits, bufs->target_bits, bufs->counters, bufs->seed,
                        bufs->episode, bufs->heuristic, bufs->mt_state, bufs->mask, bufs->mask_bits, bufs->reward,
                        bufs->terminated, bufs->invalid, bufs->solved, bufs->final_cost, bufs->final_heur, bufs->final_len,
                        bufs->reset_list, bufs->reset_count, bufs->work_list, bufs->work_count};
  for (size_t k = 0; k < sizeof(need) / sizeof(need[0]); k++) if (!need[k]) return fail(GE_E_BADARG, "a required device buffer is null");
  if (P.env_type == GE_STEINER_TREE && !bufs->rev_edge) return fail(GE_E_BADARG, "SteinerTree needs rev_edge");
  if (P.env_type == GE_DISTRIBUTION_CENTER && (!bufs->range_bits || !bufs->cover_bits)) return fail(GE_E_BADARG, "DistributionCenter needs range_bits and cover_bits");
  if (P.env_type == GE_DISTRIBUTION_CENTER && P.n <= 64 && !bufs->aux_bits) return fail(GE_E_BADARG, "DistributionCenter with n_nodes <= 64 needs aux_bits (which rows of range_bits exist)");
  if (P.env_type == GE_MULTICAST_ROUTING && P.parenting == 2 && !bufs->rev_edge) return fail(GE_E_BADARG, "MulticastRouting parenting 2 needs rev_edge");
  if (P.env_type == GE_MULTICAST_ROUTING && P.parenting >= 3 && !bufs->node_aux) return fail(GE_E_BADARG, "MulticastRouting parenting >= 3 needs node_aux");
  if (P.feat_parts > 1 && !bufs->feat_scratch) return fail(GE_E_BADARG, "feat_scratch required (ge_layout.feat_parts > 1)");
  if (P.spatial && !bufs->sw64) return fail(GE_E_BADARG, "spatial TSP needs sw64");
  if (eval_slot_bytes(P) && !bufs->eval_scratch) return fail(GE_E_BADARG, "is_eval_env of TSP / unweighted MaxIndependentSet / SteinerTree (1 < n_dests < n - 1) needs eval_scratch (ge_layout.eval_scratch_bytes)");
  if (P.W == 1 && !bufs->node_rec) return fail(GE_E_BADARG, "n_nodes <= 64 needs node_rec");
  if (prunes(P) && P.W > GE_MAXW && !bufs->prune_scratch)
    return fail(GE_E_BADARG, "parenting >= 2 on more than 512 nodes needs prune_scratch ([B, 4, W] uint64)");
  return GE_OK;
}

// SteinerTree / MulticastRouting whose mask rows fit the LDS stage of the quad-per-slot kernel (ge_step.h, ge_k_step_edge); a
// multi-class engine stages every row with the stride of its widest class (e->aw_max) and node sets of its widest class (e->P.W)
static bool edge_quad(const ge_engine *e) {
  static const bool off = getenv("GE_NO_EDGE_QUAD") != nullptr;  // diagnostic: the thread-per-slot kernel (before / after measurements)
  return !off && (e->P.env_type == GE_STEINER_TREE || e->P.env_type == GE_MULTICAST_ROUTING) && ge_edge_fits(e->aw_max, e->P.W);
}

static bool path64(const ge_engine *e) {
  return e->n_classes == 0 && (e->P.env_type == GE_SHORTEST_PATH || e->P.env_type == GE_LONGEST_PATH) && e->P.W == 1 && e->P.parenting < 2;
}

// The only place where an engine becomes kernel instantiations (e->P, e->n_classes and e->aw_max are final).  `if constexpr` keeps
// the set of instantiations to the ones an engine can run: the library is one translation unit and every extra kernel costs build time.
template <bool RAGGED, class T>
static void select_policy_kernels(GeKernels &k, int dtype) {
  k.policy_head[dtype][GE_POL_SAMPLE] = ge_k_policy_head<RAGGED, GE_POL_SAMPLE, T>;
  k.policy_head[dtype][GE_POL_GREEDY] = ge_k_policy_head<RAGGED, GE_POL_GREEDY, T>;
  k.policy_head[dtype][GE_POL_EVALUATE] = ge_k_policy_head<RAGGED, GE_POL_EVALUATE, T>;
  k.policy_grad[dtype] = ge_k_policy_grad<RAGGED, T>;
}

template <int ENV, bool RAGGED>
static void select_kernels(ge_engine *e) {
  GeKernels &k = e->k;
  k.reset = ge_k_reset<ENV, RAGGED>;
  k.features = ge_k_features<RAGGED>;
  k.features64 = ge_k_features64<RAGGED>;
  k.feat_combine = ge_k_feat_combine<RAGGED>;
  k.swap = ge_k_swap<RAGGED>;
  k.sample = ge_k_sample<RAGGED>;
  select_policy_kernels<RAGGED, float>(k, GE_LOGITS_F32);
  select_policy_kernels<RAGGED, ge_bf16>(k, GE_LOGITS_BF16);
  select_policy_kernels<RAGGED, ge_f16>(k, GE_LOGITS_F16);
  k.dc_range = ge_k_dc_range<RAGGED>;
  k.tsp_closure = ge_k_tsp_closure<RAGGED>;
  k.tsp_tour = ge_k_tsp_tour<RAGGED>;
  k.mis_baseline = ge_k_mis_baseline<RAGGED>;
  k.steiner_baseline = ge_k_steiner_baseline<RAGGED>;
  // thread-per-slot step kernel: the LDS stage holds one node set per slot of the workgroup (multi-class engine: of the widest class)
  k.step[0] = ge_k_step<ENV, false, RAGGED, 0>; k.step[1] = ge_k_step<ENV, true, RAGGED, 0>;
  k.step_threads = GE_STEP_BLOCK;
  k.step_lds = (size_t)GE_STEP_BLOCK * e->P.W * 8 + GE_STEP_BLOCK + 64;
  if constexpr (ENV == GE_STEINER_TREE || ENV == GE_MULTICAST_ROUTING) {
    if (edge_quad(e)) {
      k.step[0] = ge_k_step_edge<ENV, false, RAGGED>; k.step[1] = ge_k_step_edge<ENV, true, RAGGED>;
      k.step_quad = true;
      k.step_threads = GE_EDGE_THREADS;
      k.step_lds = ge_edge_lds_bytes(e->aw_max, e->P.W) + (RAGGED ? GE_EDGE_CLASS_BYTES : 0);  // (+ the class of every slot of the workgroup)
    }
  }
  // parenting >= 2 (multi-class engine: PRUNE 1 when every class fits GE_MAXW words, else PRUNE 2 for all of them -- e->P.W is the
  // widest class's)
  if constexpr (ENV == GE_LONGEST_PATH || ENV == GE_TSP) {
    if (prunes(e->P) && e->P.W > GE_MAXW) { k.step[0] = ge_k_step<ENV, false, RAGGED, 2>; k.step[1] = ge_k_step<ENV, true, RAGGED, 2>; }
    else if (prunes(e->P)) { k.step[0] = ge_k_step<ENV, false, RAGGED, 1>; k.step[1] = ge_k_step<ENV, true, RAGGED, 1>; }
  }
  if constexpr (!RAGGED) {
    if (path64(e)) {
      k.step_path64[0][0] = ge_k_step_path64<false, false>; k.step_path64[0][1] = ge_k_step_path64<false, true>;
      k.step_path64[1][0] = ge_k_step_path64<true, false>; k.step_path64[1][1] = ge_k_step_path64<true, true>;
    }
  }
}

// the dynamic-LDS limit of a kernel the engine selected, for the byte count it is launched with
static bool raise_lds(const void *kernel, size_t bytes) {
  (void)kernel;
  return bytes <= 64 * 1024 || (hipError_t)GE_SET_MAX_DYN_LDS(kernel, bytes) == hipSuccess;
}

// kernels, the launch plan and the LDS limits from e->P (uniform engine) or from the class table (multi-class engine)
static int finish_create(ge_engine *e) {
  const GeParams &P = e->P;
  const bool rg = e->n_classes > 0;
  const int nblk = step_blocks(P.B), pre2 = prefix_bytes(P.B);
  GE_FOR_ENV(P.env_type, if (rg) (select_kernels<ENV, true>(e)); else (select_kernels<ENV, false>(e)));
  GePlan &L = e->plan;
  // a multi-class launch keeps the queue prefix BEHIND the widest carve of the bucket's classes (a class's own carve places it for
  // that class alone); the carve of a uniform engine holds it
  auto behind = [&](int body, int &pre) { pre = ge_align16(body); return pre + pre2; };
  const GeParams *first = rg ? e->classes.data() : &e->P;
  const int n_classes = rg ? e->n_classes : 1;
  L.n_buckets = rg ? GE_MAX_BUCKETS : 1;
  int graph_lds = 0, gen_lds = 0;   // the largest launch of the graph kernel and of the generic feature kernel
  int gen_body = 0, f64_body = 0;  // the largest carve of a class on the generic kernel; the fast path's item bodies
  for (int b = 0; b < L.n_buckets; b++) {
    GeBucket &K = L.bk[b];
    int graph = 0, gen = 0, all = 0, waves = 1;
    for (const GeParams *C = first; C < first + n_classes; C++) {
      if (C->bucket != b) continue;
      K.used = true;
      if (C->lds.total > graph) graph = C->lds.total;
      if (C->ldsf.total > all) all = C->ldsf.total;
      if (takes_generic(*C)) { if (C->ldsf.total > gen) gen = C->ldsf.total; if (C->ldsf.waves > waves) waves = C->ldsf.waves; }
      else { L.feat_fast = true; const int body = ge_f64_pre_off(C->E, C->env_type == GE_TSP, nblk); if (body > f64_body) f64_body = body; }
    }
    if (!K.used) continue;
    K.list_only = gen == 0;
    if (gen > gen_body) gen_body = gen;
    // ---- graph kernel
    K.graph.grid = resident_grid(graph, P.B);
    K.graph.pre = P.lds.pre; K.graph.lds = graph;
    if (rg && P.lds.pre != 0) K.graph.lds = behind(graph, K.graph.pre);  // (else the prefix overlays the generator state at the head of every carve)
    if (K.graph.lds > graph_lds) graph_lds = K.graph.lds;
    // ---- generic feature kernel: the wave count every class of the bucket can hold (a class's surplus waves do not search,
    // ge_features_generic_env); list_only: one wave per slot (ge_make_ldsf: n <= 64), sized for the bucket's largest class
    K.gen.threads = GE_WAVE * waves;
    K.gen.pre_off = P.ldsf.pre; K.gen.lds = P.ldsf.total;
    if (rg) K.gen.lds = behind(K.list_only ? all : gen, K.gen.pre_off);
    K.gen.grid = resident_grid(K.gen.lds, P.B);
    // (the fallback list is normally empty and a handful of slots at most: eight workgroups dispatch in less time than 64 -- the
    // launch is on every step's critical path)
    if (K.list_only && (rg || K.gen.grid > 8)) K.gen.grid = 8;
    if (K.gen.lds > gen_lds) gen_lds = K.gen.lds;
  }
  if (!rg) L.inject = inject_carve(P, P.B);  // (ge_inject_state is not built for the multi-class engine)
  if (!carves_fit({graph_lds, L.inject.total, gen_lds})) return fail(GE_E_TOOBIG, "per-env graph does not fit 160 KiB of LDS");
  L.nseed = (resident_grid(graph_lds, P.B) + 63) / 64;  // one seeding workgroup per 64 regenerating workgroups: the usual queue fits one round of both
  if (!raise_lds((const void *)e->k.reset, graph_lds > L.inject.total ? graph_lds : L.inject.total)) return fail(GE_E_LAUNCH, "cannot raise the dynamic LDS limit of the reset kernel");
  // ---- step kernel: the quad-per-slot stage of the edge-action envs (mask rows + node sets of 256 slots) passes 64 KB; the
  // thread-per-slot stage (one node set per slot of the workgroup) would above 2 048 nodes
  if (!raise_lds((const void *)e->k.step[0], e->k.step_lds) || !raise_lds((const void *)e->k.step[1], e->k.step_lds))
    return fail(GE_E_LAUNCH, e->k.step_quad ? "cannot raise the dynamic LDS limit of the edge step kernel" : "cannot raise the dynamic LDS limit of the step kernel");
  // ---- n <= 64 feature kernel: the item bodies (the queue prefix overlays them), then the tail {item slots, overflow flag}
  L.f64_pre_off = ge_align16(f64_body);
  L.f64_lds = L.feat_fast ? L.f64_pre_off + GE_F64_ITEMS * 4 * 4 + 16 : 0;
  // ---- split seeding: as many pass-2 workgroups as cover the slots of the graph launch's seeding workgroups in one trip; a
  // pass-2 workgroup's tiles lie inside the feature launch's carve (the headline's is larger: nothing changes there)
  L.nseed2 = (GE_SEED_SPLIT && !rg && L.feat_fast) ? (L.nseed * GE_WAVE + GE_SEED2_ITEMS - 1) / GE_SEED2_ITEMS : 0;
  const int seed2_lds = GE_SEED2_WAVES * GE_SEED2_WAVE_BYTES;
  if (L.nseed2 > 0 && L.f64_lds < seed2_lds) L.f64_lds = seed2_lds;
  if (!carves_fit({L.f64_lds})) return fail(GE_E_TOOBIG, "feature kernel does not fit LDS");
  if (!raise_lds((const void *)e->k.features, gen_lds)) return fail(GE_E_LAUNCH, "cannot raise the dynamic LDS limit of the feature kernel");
  if (L.feat_fast && !raise_lds((const void *)e->k.features64, L.f64_lds)) return fail(GE_E_LAUNCH, "cannot raise the dynamic LDS limit of the n<=64 feature kernel");
  L.feat_grid = resident_grid(L.feat_fast ? L.f64_lds : gen_body, P.B);
  // ---- policy head: one lane group per row, the same width for every row of the launch (a slot finds its class through slot_class,
  // so the rows a wave holds follow from the slot numbers alone); above 32 actions in any class a wave per row
  int a_max = 0;
  for (const GeParams *C = first; C < first + n_classes; C++) if (C->A > a_max) a_max = C->A;
  L.pol_group = 4;
  while (L.pol_group < 64 && L.pol_group < a_max) L.pol_group <<= 1;
  const int64_t waves = ((int64_t)P.B * L.pol_group + GE_WAVE - 1) / GE_WAVE;
  L.pol_grid = (int)((waves + GE_POL_THREADS / GE_WAVE - 1) / (GE_POL_THREADS / GE_WAVE));
  return GE_OK;
}

extern "C" int ge_create(const ge_config *cfg, const ge_buffers *bufs, ge_engine **out) {
  if (!bufs || !out) return fail(GE_E_BADARG, "null argument");
  GeParams P;
  int rc = derive(cfg, P);
  if (rc != GE_OK) return rc;
  rc = check_buffers(P, bufs);
  if (rc != GE_OK) return rc;
  P.buf = *bufs;
  std::unique_ptr<ge_engine> e(new (std::nothrow) ge_engine());
  if (!e) return fail(GE_E_BADARG, "out of host memory");
  e->P = P; e->cfg = *cfg; e->aw_max = P.AW;
  rc = finish_create(e.get());
  if (rc == GE_OK) *out = e.release();
  return rc;
}

// (sizeof(GeParams) includes policy_off, the class's place in the policy head's flat logits)
extern "C" int64_t ge_ragged_table_bytes(int32_t n_classes) { return (int64_t)sizeof(GeParams) * (n_classes > 0 ? n_classes : 0); }

extern "C" int ge_create_ragged(const ge_config *cfgs, const ge_buffers *bufs, int32_t n_classes, void *class_table,
                                int32_t *slot_class, int32_t *class_start, ge_engine **out) {
  if (!cfgs || !bufs || !out || !class_table || !slot_class || !class_start || n_classes < 1) return fail(GE_E_BADARG, "null argument");
  const int t = cfgs[0].env_type;
  int64_t total = 0;
  for (int c = 0; c < n_classes; c++) total += cfgs[c].num_envs;
  if (total > 8192 * GE_STEP_BLOCK) return fail(GE_E_TOOBIG, "num_envs > 2M per engine");
  std::unique_ptr<ge_engine> e(new (std::nothrow) ge_engine());
  if (!e) return fail(GE_E_BADARG, "out of host memory");
  e->classes.resize(n_classes);
  std::vector<int32_t> start(n_classes + 1, 0), cls_of((size_t)total);
  int widest = 0, aw_max = 0;
  int64_t policy_off = 0;
  for (int c = 0; c < n_classes; c++) {
    GeParams &C = e->classes[c];
    int rc = derive(&cfgs[c], C, (int)total);
    if (rc == GE_OK) rc = check_buffers(C, &bufs[c]);
    if (rc == GE_OK && (cfgs[c].env_type != t || cfgs[c].autoreset != cfgs[0].autoreset || cfgs[c].seed_stride != cfgs[0].seed_stride))
      rc = fail(GE_E_BADARG, "the classes of a multi-class engine share env_type, autoreset and seed_stride");
    if (rc == GE_OK && (cfgs[c].weighted != cfgs[0].weighted || cfgs[c].parenting != cfgs[0].parenting || cfgs[c].spatial != cfgs[0].spatial ||
                        cfgs[c].is_eval_env != cfgs[0].is_eval_env))
      rc = fail(GE_E_BADARG, "the classes of a multi-class engine share weighted, parenting, spatial and is_eval_env (they differ in n, m and the per-instance scalars only)");
    if (rc == GE_OK && (cfgs[c].env_index_base != cfgs[0].env_index_base + start[c] || bufs[c].seed != bufs[0].seed + start[c] ||
                        bufs[c].episode != bufs[0].episode + start[c] || bufs[c].mt_state != bufs[0].mt_state + (int64_t)start[c] * GE_SEED_DEPTH * 2 * GE_MT_N))
      rc = fail(GE_E_BADARG, "classes follow one another in slot order: env_index_base, seed, episode and mt_state of class c start at its first global slot");
    // the engine-wide kernels take the queues and the work lists from class 0 and index slot_rec by global slot through the class's pointer
    if (rc == GE_OK && (bufs[c].reset_list != bufs[0].reset_list || bufs[c].reset_count != bufs[0].reset_count || bufs[c].work_list != bufs[0].work_list ||
                        bufs[c].work_count != bufs[0].work_count || bufs[c].slot_rec != bufs[0].slot_rec + 2 * (int64_t)start[c]))
      rc = fail(GE_E_BADARG, "reset_list, reset_count, work_list and work_count are engine-wide (the same pointers in every class), and slot_rec of class c starts at its first global slot");
    if (rc != GE_OK) return rc;
    C.buf = bufs[c];
    C.policy_off = policy_off; policy_off += (int64_t)C.B * C.A;
    start[c + 1] = start[c] + cfgs[c].num_envs;
    for (int i = start[c]; i < start[c + 1]; i++) cls_of[(size_t)i] = c;
    if (C.n > e->classes[widest].n) widest = c;
    if (C.AW > aw_max) aw_max = C.AW;
  }
  // parenting >= 2 of LongestPath / TSP: one PRUNE form for the whole engine -- the walks in memory (PRUNE 2) as soon as one class is
  // above GE_MAXW words, and then every class needs its prune_scratch (ge_layout reports none for a class that would fit registers)
  if (prunes(e->classes[widest]) && e->classes[widest].W > GE_MAXW)
    for (int c = 0; c < n_classes; c++)
      if (!bufs[c].prune_scratch) return fail(GE_E_BADARG, "parenting >= 2 with a class above 512 nodes runs the residual-graph walks in memory for every class: each class needs prune_scratch ([B_c, 4, W_c] uint64)");
  // the classes of an LDS bucket share one launch of the generic feature kernel (the plan: finish_create).  Every class takes the
  // wave count it would choose as a uniform engine -- two workgroups per CU where that leaves at least four waves, else one; if the
  // bucket's widest allocation then leaves room for ONE workgroup per CU only, the smaller classes are re-derived for the whole CU
  // (up to 16 waves: idle LDS otherwise)
  for (int b = 0; b < GE_MAX_BUCKETS; b++) {
    for (int pass = 0; pass < 2; pass++) {
      int gen_lds = 0;
      for (GeParams &C : e->classes) if (bucket_of(C.n) == b) {
        C.bucket = b;
        if (pass == 0) ge_make_ldsf(C, (int)total); else ge_make_ldsf(C, (int)total, 0, 160 * 1024 - 2048);
        ge_tune_feat_parts(C);
        if (takes_generic(C) && C.ldsf.total > gen_lds) gen_lds = C.ldsf.total;
      }
      if (2 * (gen_lds + prefix_bytes(total)) <= kMaxLds) break;  // two workgroups per CU: the classes keep their own choice
    }
  }
  // engine-wide block: the widest class's geometry (LDS stage of the step kernel), all slots, the global arrays of class 0
  e->P = e->classes[widest];
  e->P.B = (int32_t)total;
  for (const GeParams &C : e->classes) if (C.feat_parts > e->P.feat_parts) e->P.feat_parts = C.feat_parts;
  e->P.buf = bufs[0];
  e->P.env_index_base = cfgs[0].env_index_base;
  e->P.policy_off = 0;
  e->cfg = cfgs[0]; e->cfg.num_envs = (int32_t)total;
  e->n_classes = n_classes;
  e->aw_max = aw_max;
  e->P.AW = aw_max;  // (the edge step kernel's LDS stage: the widest mask row, which for the edge-action envs need not be the widest class's)
  if (hipMemcpy(class_table, e->classes.data(), sizeof(GeParams) * (size_t)n_classes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(slot_class, cls_of.data(), sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(class_start, start.data(), sizeof(int32_t) * (size_t)(n_classes + 1), hipMemcpyHostToDevice) != hipSuccess) {
    return fail(GE_E_LAUNCH, "cannot copy the class table to the device");
  }
  e->R.classes = (const GeParams *)class_table; e->R.slot_class = slot_class; e->R.class_start = class_start; e->R.n_classes = n_classes;
  e->R.f64_tsp_e = 0;
  for (const GeParams &C : e->classes) if (C.env_type == GE_TSP && C.n <= 64 && C.E > e->R.f64_tsp_e) e->R.f64_tsp_e = C.E;
  const int rc = finish_create(e.get());
  if (rc == GE_OK) *out = e.release();
  return rc;
}

// the per-slot slabs an image must hold for this (sub-)engine
static int check_image(const GeParams &P, const ge_buffers &I) {
  const void *need[] = {I.x, I.edge_index, I.edge_attr, I.row_ptr, I.colw, I.scode, I.adj_bits, I.slot_rec, I.terminals, I.node_bits,
                        I.target_bits, I.counters, I.heuristic, I.mask, I.mask_bits};
  for (size_t k = 0; k < sizeof(need) / sizeof(need[0]); k++) if (!need[k]) return fail(GE_E_BADARG, "a required slab of the spare image is null");
  const ge_buffers &G = P.buf;
  if ((G.sw64 && !I.sw64) || (G.node_rec && !I.node_rec) || (G.rev_edge && !I.rev_edge) || (G.aux_bits && !I.aux_bits) || (G.node_aux && !I.node_aux) ||
      (G.range_bits && !I.range_bits) || (G.cover_bits && !I.cover_bits))
    return fail(GE_E_BADARG, "the spare image lacks an optional slab the engine has (sw64 / node_rec / rev_edge / aux_bits / node_aux / range_bits / cover_bits)");
  return GE_OK;
}
// V = P seen through image I: per-slot slabs from the image, everything that sequences the engine shared with the live view
static GeParams image_view(const GeParams &P, const ge_buffers &I, int32_t *refill_list, int32_t *refill_count) {
  GeParams V = P;
  ge_buffers B = I;
  const ge_buffers &G = P.buf;
  B.seed = G.seed; B.episode = G.episode; B.mt_state = G.mt_state;
  B.work_list = G.work_list; B.work_count = G.work_count; B.feat_scratch = G.feat_scratch; B.eval_scratch = G.eval_scratch;
  B.reset_list = refill_list; B.reset_count = refill_count;
  B.reward = G.reward; B.terminated = G.terminated; B.invalid = G.invalid; B.solved = G.solved;
  B.final_cost = G.final_cost; B.final_heur = G.final_heur; B.final_len = G.final_len;  // (not written by a refill)
  B.actions_out = nullptr; B.stream_state = nullptr;
  V.buf = B;
  return V;
}

extern "C" int ge_attach_spares(ge_engine *e, const ge_spares *sp, void *class_table_spare) {
  if (!e || !sp) return fail(GE_E_BADARG, "null argument");
  if (e->spares) return fail(GE_E_STATE, "spares are already attached");
  if (!e->P.autoreset) return fail(GE_E_BADARG, "spares serve autoreset: this engine freezes finished slots");
  if (e->P.buf.stream_state) return fail(GE_E_UNSUPPORTED, "spares and stream_state (reset(seed=None) continuing the streams) exclude each other: an image generated ahead of time would leave the streams of the wrong episode behind");
  if (!sp[0].state || !sp[0].swap_list || !sp[0].swap_count || !sp[0].refill_list || !sp[0].refill_count) return fail(GE_E_BADARG, "state / swap_list / swap_count / refill_list / refill_count are required");
  if (sp[0].period < 1) return fail(GE_E_BADARG, "period must be >= 1");
  if (e->n_classes > 0 && !class_table_spare) return fail(GE_E_BADARG, "a multi-class engine needs class_table_spare (ge_ragged_table_bytes)");
  int rc = GE_OK;
  if (e->n_classes == 0) rc = check_image(e->P, sp[0].image);
  for (int c = 0; c < e->n_classes && rc == GE_OK; c++) rc = check_image(e->classes[c], sp[c].image);
  if (rc != GE_OK) return rc;
  e->refill_list = sp[0].refill_list; e->refill_count = sp[0].refill_count;
  e->PS = image_view(e->P, sp[0].image, e->refill_list, e->refill_count);
  if (e->n_classes > 0) {
    e->classesS.resize(e->n_classes);
    for (int c = 0; c < e->n_classes; c++) e->classesS[c] = image_view(e->classes[c], sp[c].image, e->refill_list, e->refill_count);
    if (hipMemcpy(class_table_spare, e->classesS.data(), sizeof(GeParams) * (size_t)e->n_classes, hipMemcpyHostToDevice) != hipSuccess)
      return fail(GE_E_LAUNCH, "cannot copy the spare class table to the device");
    e->RS = e->R; e->RS.classes = (const GeParams *)class_table_spare;
  }
  e->P.spare_state = sp[0].state; e->P.swap_list = sp[0].swap_list; e->P.swap_count = sp[0].swap_count;
  e->PS.spare_state = sp[0].state;
  e->period = sp[0].period; e->pending_calls = 0;
  // a slot's image is some tens of KB: split it over workgroups so that a handful of finished slots is not a handful of workgroups
  const GeParams &P = e->P;
  const int64_t slot_bytes = (int64_t)P.n * P.F * 4 + (int64_t)P.E * (16 + 4 * P.Fe + 2 + 1 + (P.buf.rev_edge ? 4 : 0)) + (int64_t)P.n * P.W * 8 * (P.buf.range_bits ? 2 : 1) + P.A;
  int parts = (int)(slot_bytes / 8192); if (parts < 1) parts = 1; if (parts > 16) parts = 16;
  if (parts >= 4) parts = GE_SWAP_GROUPS;  // a large image: one workgroup per (group of) whole arrays
  e->swap_parts = parts;
  e->spares = true;
  e->plan.nseed2 = 0;  // an engine with spares seeds two episodes ahead from refill and in-place launches alike: unsplit
  // (the caller zeroes `state`; ge_reset / ge_inject_state clear it and refill every image)
  return GE_OK;
}

extern "C" int ge_destroy(ge_engine *e) {
  if (!e) return GE_OK;
  if (e->have_events) for (int k = 0; k < 4; k++) (void)hipEventDestroy(e->ev[k]);
  delete e;
  return GE_OK;
}

static int check_launch(const char *what) {
  // GE_DEBUG_SYNC=1: wait for every launch and name it (a kernel fault is otherwise reported at some later synchronisation)
  static const bool debug_sync = getenv("GE_DEBUG_SYNC") != nullptr;
  if (debug_sync) {
    fprintf(stderr, "[graphenvs] %s ...\n", what); fflush(stderr);
    const hipError_t hs = hipDeviceSynchronize();  // an asynchronous fault of THIS launch surfaces here
    fprintf(stderr, "[graphenvs] %s %s\n", what, hs == hipSuccess ? "done" : hipGetErrorString(hs)); fflush(stderr);
    if (hs != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: %s (GE_DEBUG_SYNC)", what, hipGetErrorString(hs)); return GE_E_LAUNCH; }
  }
  hipError_t hr = hipGetLastError();
  if (hr != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(hr)); return GE_E_LAUNCH; }
  return GE_OK;
}

// ring entries jlo .. GE_SEED_DEPTH - 1 of every slot from seeds[] (+ j * seed_stride), on the caller's stream
static int launch_seed(ge_engine *e, const uint32_t *seeds, int jlo, void *stream) {
  const int64_t items = (int64_t)(GE_SEED_DEPTH - jlo) * e->P.B;
  int64_t grid = (items + GE_WAVE - 1) / GE_WAVE;
  if (grid > 8192) grid = 8192;
  GE_LAUNCH(ge_k_seed, (int)grid, 2 * GE_WAVE, GE_SEED_LDS_BYTES, stream, e->P, seeds, jlo);
  return check_launch("seed kernel");
}

// V: the engine (e->P) or its spare-image view (e->PS); VR: the matching class table
static int launch_combine(ge_engine *e, const GeParams &V, const GeRagged &VR, GeRun run, bool small, void *stream) {
  int64_t items = (int64_t)(run.items == GE_ITEMS_ALL ? V.B : (small ? 64 : 4096)) * V.n;
  int grid = (int)((items + 255) / 256); if (grid > 8192) grid = 8192;
  GE_LAUNCH(e->k.feat_combine, grid, 256, prefix_bytes(V.B), stream, V, VR, run);
  return check_launch("feature combine kernel");
}

// a launch over every slot spreads to four times the resident grid, one workgroup per slot at most; a queue launch strides over its list
static int spread(int grid, int B, bool queue) { return queue ? grid : (B < grid * 4 ? B : grid * 4); }

// `small`: the queue is expected to be short (the in-place regenerations of an engine with spares): a fraction of the grid
static int fast_grid(const ge_engine *e, int B, bool queue, bool small) {
  const int g = spread(e->plan.feat_grid, B, queue);
  return small && g > 64 ? 64 : g;
}

// workgroups of the generic feature kernel's launch for bucket K.  With the fast path in front (plan.feat_fast) the launch takes
// the fallback list: every slot of a class with n > 64, or -- K.list_only -- the rare slots too deep for the fast path
static int generic_grid(const ge_engine *e, const GeBucket &K, const GeParams &V, GeRun run, bool small) {
  const bool queue = run.items == GE_ITEMS_QUEUE, list = e->plan.feat_fast;
  if (K.list_only) return K.gen.grid;
  int64_t want = list ? (int64_t)K.gen.grid * (queue ? 1 : 4) : fast_grid(e, V.B, queue, small);
  want *= ge_feat_workgroups(V.feat_parts);
  if (!list && queue && !run.refill && want > 4608) want = 4608;  // the list is short, workgroups stride over it
  if (small && want > 288) want = 288;
  return want > 65535 * 16 ? 65535 * 16 : (int)want;
}

static int launch_features(ge_engine *e, const GeParams &V, const GeRagged &VR, GeRun run, bool small, void *stream) {
  const GePlan &L = e->plan;
  const GeRun rest = L.feat_fast ? as_list(run) : run;  // behind the fast path: its fallback list
  int rc = GE_OK;
  if (L.feat_fast) {
    // split seeding: the pass-2 workgroups come out of the launch's resident grid, not on top of it -- a workgroup beyond the
    // resident round starts when another ends, i.e. runs its items as a tail behind the launch (one engine: 123 -> 141 us)
    const bool queue = run.items == GE_ITEMS_QUEUE;
    const int nseed2 = queue ? run.seed_split : 0;
    int grid = fast_grid(e, V.B, queue, small) - nseed2;
    if (grid < 1) grid = 1;
    GE_LAUNCH(e->k.features64, grid + nseed2, GE_F64_THREADS, L.f64_lds, stream, V, VR, run, L.f64_pre_off);
    rc = check_launch("feature kernel (n <= 64)");
  }
  for (int b = 0; b < L.n_buckets && rc == GE_OK; b++) {  // one launch per LDS bucket
    const GeBucket &K = L.bk[b];
    if (!K.used) continue;
    GE_LAUNCH(e->k.features, generic_grid(e, K, V, run, small), K.gen.threads, K.gen.lds, stream, V, VR, rest, K.gen.pre_off, e->n_classes > 0 ? b : -1);
    rc = check_launch(L.feat_fast ? "feature kernel (fallback list)" : "feature kernel");
  }
  if (rc != GE_OK || V.feat_parts == 1) return rc;
  return launch_combine(e, V, VR, rest, small, stream);
}

// is_eval_env baselines that are sequential programs (ge_tsp_eval.h: TSP Christofides, MaxIndependentSet clique removal, SteinerTree
// Kou) for the regenerated slots, on the slabs the graph kernel wrote.  Multi-class engine: one launch over all slots; every item
// finds its class and runs on that class's eval_scratch (VR: the live or the spare class table)
static int launch_seq_baseline(ge_engine *e, const GeParams &P, const GeRagged &VR, int queue, void *stream) {
  const uint64_t slot_bytes = e->n_classes > 0 ? 0 : eval_slot_bytes(P);
  const int pre = prefix_bytes(P.B);
  int g = (P.B + GE_TSP_EVAL_THREADS - 1) / GE_TSP_EVAL_THREADS; if (g > 4096) g = 4096;  // one thread per item
  if (P.env_type == GE_MAX_INDEPENDENT_SET) {
    GE_LAUNCH(e->k.mis_baseline, g, GE_TSP_EVAL_THREADS, pre, stream, P, VR, queue, (uint8_t *)P.buf.eval_scratch, slot_bytes);
    return check_launch("MaxIndependentSet baseline kernel");
  }
  if (P.env_type == GE_STEINER_TREE) {
    GE_LAUNCH(e->k.steiner_baseline, g, GE_TSP_EVAL_THREADS, pre, stream, P, VR, queue, (uint8_t *)P.buf.eval_scratch, slot_bytes);
    return check_launch("SteinerTree baseline kernel");
  }
  const int pre_off = GE_WAVE * P.W * 8;  // (P.W: the widest class's in a multi-class engine)
  GE_LAUNCH(e->k.tsp_closure, P.B < 2048 ? P.B : 2048, GE_TSP_EVAL_THREADS, pre_off + pre, stream, P, VR, queue, (uint8_t *)P.buf.eval_scratch, slot_bytes, pre_off);
  int rc = check_launch("TSP baseline: closure kernel");
  if (rc != GE_OK) return rc;
  GE_LAUNCH(e->k.tsp_tour, g, GE_TSP_EVAL_THREADS, pre, stream, P, VR, queue, (uint8_t *)P.buf.eval_scratch, slot_bytes);
  return check_launch("TSP baseline: tour kernel");
}

// One pass of the reset path over the items `run` names, on the engine (V = e->P) or on its spare image (V = e->PS, run.refill).
// Everything on the caller's stream, in order: generator states (full reset: the ring of every slot; queue launches: seeding
// workgroups inside the reset launch), graph kernel, sequential baselines, feature kernel(s).
static int launch_reset(ge_engine *e, const GeParams &V, const GeRagged &VR, const uint32_t *seeds, GeRun run, const GeInject &inj, bool small, void *stream) {
  int rc = GE_OK;
  const bool queue = run.items == GE_ITEMS_QUEUE;
  if (run.restart == 1) rc = launch_seed(e, seeds, 0, stream);
  else if (run.restart == 2) rc = launch_seed(e, inj.seeds, 1, stream);  // the injected episode needs no states of its own
  if (rc != GE_OK) return rc;
  if (run.cont) {
    int64_t g = ((int64_t)V.B + GE_WAVE - 1) / GE_WAVE; if (g > 8192) g = 8192;
    GE_LAUNCH(ge_k_seed_next, (int)g, 2 * GE_WAVE, GE_SEED_LDS_BYTES, stream, V);
    rc = check_launch("seed kernel (next ring entry)");
    if (rc != GE_OK) return rc;
  }
  const GePlan &L = e->plan;
  int nseed = queue ? L.nseed : 0;
  if (small && nseed > 2) nseed = 2;
  GeParams V2 = V;  // the view with the launch's own carve: the plan's values, nothing is derived here
  if (run.inject) { V2.nocolw = 0; V2.nowsort = 0; }  // the injected rows come in the caller's order: this launch keeps the {neighbour, code} list
  for (int b = 0; b < L.n_buckets && rc == GE_OK; b++) {  // one launch per LDS bucket
    const GeBucket &K = L.bk[b];
    if (!K.used) continue;
    int g = spread(K.graph.grid, V.B, queue), lds = K.graph.lds;
    if (small && g > 128) g = 128;
    V2.lds.pre = K.graph.pre;
    if (run.inject) { V2.lds = L.inject; lds = L.inject.total; }
    GE_LAUNCH(e->k.reset, g + nseed, GE_RESET_THREADS, lds, stream, V2, VR, seeds, run, inj, nseed, e->n_classes > 0 ? b : -1);
    rc = check_launch("reset kernel");
    nseed = 0;  // the seeding workgroups ride in the first launch
  }
  if (rc != GE_OK) return rc;
  bool baseline = eval_slot_bytes(V) != 0;
  for (const GeParams &C : e->classes) baseline = baseline || eval_slot_bytes(C) != 0;  // (SteinerTree: Kou depends on the class's n_dests)
  if (!run.inject && baseline) rc = launch_seq_baseline(e, V, VR, queue ? 1 : 0, stream);
  if (rc != GE_OK) return rc;
  if (!run.inject) rc = launch_features(e, V, VR, run, small, stream);
  if (rc == GE_OK && run.restart) e->seeded = true;
  if (rc == GE_OK && run.restart == 1 && e->P.buf.stream_state) e->streams = true;
  return rc;
}

// every image is empty; with seeded generator states refill them all right away (one pass at full occupancy)
static int refill_spares(ge_engine *e, void *stream) {
  GE_LAUNCH(ge_k_refill_list, step_blocks(e->P.B), GE_STEP_BLOCK, 64, stream, e->P, e->refill_list, e->refill_count);
  int rc = check_launch("refill list kernel");
  if (rc != GE_OK) return rc;
  e->pending_calls = 0;
  return launch_reset(e, e->PS, e->RS, nullptr, run_refill(), kNoInject, false, stream);
}
static int invalidate_spares(ge_engine *e, void *stream) {
  if (!e->spares) return GE_OK;
  if (hipMemsetAsync(e->P.spare_state, 0, (size_t)e->P.B, (hipStream_t)stream) != hipSuccess) return fail(GE_E_LAUNCH, "hipMemsetAsync failed");
  return (e->seeded && e->P.autoreset) ? refill_spares(e, stream) : GE_OK;
}

// a full reset / injection leaves the finished-slot queues empty: the regeneration queue and, with spares, the swap queue (next-step
// autoreset consumes it at the START of the next ge_step: a stale entry would copy an image over the slot that was just reset)
static int clear_queue(ge_engine *e, void *stream) {
  const size_t bytes = sizeof(int32_t) * (size_t)step_blocks(e->P.B);
  if (hipMemsetAsync(e->P.buf.reset_count, 0, bytes, (hipStream_t)stream) != hipSuccess) return fail(GE_E_LAUNCH, "hipMemsetAsync failed");
  if (e->spares && hipMemsetAsync(e->P.swap_count, 0, bytes, (hipStream_t)stream) != hipSuccess) return fail(GE_E_LAUNCH, "hipMemsetAsync failed");
  return GE_OK;
}

extern "C" int ge_reset(ge_engine *e, const uint32_t *seeds, void *stream) {
  if (!e || !seeds) return fail(GE_E_BADARG, "null argument");
  int rc = clear_queue(e, stream);
  if (rc != GE_OK) return rc;
  rc = launch_reset(e, e->P, e->R, seeds, run_full(), kNoInject, false, stream);
  if (rc == GE_OK) e->loaded = true;
  if (rc == GE_OK) rc = invalidate_spares(e, stream);  // ... and refill: every slot's episode 1 waits in its image
  return rc;
}

extern "C" int ge_reset_continue(ge_engine *e, void *stream) {
  if (!e) return fail(GE_E_BADARG, "null argument");
  if (e->n_classes > 0) return fail(GE_E_UNSUPPORTED, "ge_reset_continue is not built for the multi-class engine");
  if (e->spares) return fail(GE_E_UNSUPPORTED, "ge_reset_continue on an engine with spares: an image generated ahead of time would leave the streams of the wrong episode behind");
  if (!e->P.buf.stream_state) return fail(GE_E_STATE, "ge_reset_continue needs ge_buffers.stream_state (the streams every reset leaves behind)");
  if (!e->loaded || !e->seeded || !e->streams) return fail(GE_E_STATE, "ge_reset_continue before ge_reset: there is no stream to continue");
  int rc = clear_queue(e, stream);
  if (rc != GE_OK) return rc;
  return launch_reset(e, e->P, e->R, nullptr, run_continue(), kNoInject, false, stream);
}

extern "C" int ge_inject_state(ge_engine *e, const int64_t *links, const uint8_t *wcode, const float *x,
                               const int32_t *terminals, const uint32_t *seeds, void *stream) {
  if (!e || !links || !wcode || !x) return fail(GE_E_BADARG, "null argument");
  if (e->n_classes > 0) return fail(GE_E_UNSUPPORTED, "ge_inject_state is not built for the multi-class engine (inject into uniform engines)");
  const int t = e->P.env_type;
  if ((t == GE_SHORTEST_PATH || t == GE_LONGEST_PATH || t == GE_STEINER_TREE || t == GE_MULTICAST_ROUTING || t == GE_DISTRIBUTION_CENTER ||
       t == GE_PERISHABLE_DELIVERY) && !terminals)
    return fail(GE_E_BADARG, "terminals required (source / destinations, targets, or pickups then drop-offs)");
  if (!seeds && e->P.autoreset && !e->seeded)
    return fail(GE_E_STATE, "ge_inject_state without seeds on an engine with autoreset whose generator states were never seeded: pass seeds, or call ge_reset first");
  GeInject inj = {links, wcode, x, terminals, seeds};
  int rc = clear_queue(e, stream);  // slots queued before the injection must not be regenerated over the injected state
  if (rc != GE_OK) return rc;
  rc = launch_reset(e, e->P, e->R, nullptr, run_inject(seeds != nullptr), inj, false, stream);
  if (rc == GE_OK) e->loaded = true;
  if (rc == GE_OK) rc = invalidate_spares(e, stream);  // the images belong to the episodes that follow the injected ones
  return rc;
}

extern "C" int ge_sample_actions(ge_engine *e, uint64_t policy_seed, int64_t *actions, void *stream);

// the step kernel the engine selected; sample: the fused device policy draws the actions from policy_seed, else they are `actions`
static void launch_step(ge_engine *e, bool sample, const int64_t *actions, uint64_t policy_seed, void *stream) {
  const GeKernels &k = e->k;
  const int grid = step_blocks(e->P.B);
  if (path64(e)) GE_LAUNCH(k.step_path64[sample][e->spares], grid, k.step_threads, k.step_lds, stream, e->P, actions, policy_seed);
  else GE_LAUNCH(k.step[sample], grid, k.step_threads, k.step_lds, stream, e->P, e->R, actions, policy_seed);
}

// DistributionCenter with n <= 64 (in a multi-class engine: in any class) computes a centre's coverage range when it is chosen
static bool dc_range(const ge_engine *e) {
  if (e->P.env_type != GE_DISTRIBUTION_CENTER) return false;
  if (e->n_classes == 0) return e->P.n <= 64;
  for (const GeParams &C : e->classes) if (C.n <= 64) return true;
  return false;
}

// call-order guard (the reference raises in the same situations): stepping needs an episode in the slots, and autoreset needs a
// seeded generator ring -- an unseeded MT19937 state would draw the same node pair for ever
static int check_state(const ge_engine *e) {
  if (!e->loaded) return fail(GE_E_STATE, "the engine holds no episode yet: call ge_reset (or ge_inject_state) first");
  if (e->P.autoreset && !e->seeded) return fail(GE_E_STATE, "autoreset needs seeded generator states: call ge_reset, or ge_inject_state with seeds");
  return GE_OK;
}

extern "C" int ge_step_only(ge_engine *e, const int64_t *actions, void *stream) {
  if (!e || !actions) return fail(GE_E_BADARG, "null argument");
  int rc = check_state(e);
  if (rc != GE_OK) return rc;
  if (dc_range(e)) {  // the chosen centres' coverage ranges, computed when they are chosen
    const int rows = e->n_classes > 0 ? 64 : e->P.n;  // distance columns per lane (multi-class engine: of the largest class that takes this path)
    GE_LAUNCH(e->k.dc_range, (e->P.B + GE_WAVE - 1) / GE_WAVE, GE_WAVE, (size_t)rows * GE_WAVE * 8 + GE_WAVE * 64, stream, e->P, e->R, actions);
    rc = check_launch("coverage range kernel");
    if (rc != GE_OK) return rc;
  }
  launch_step(e, false, actions, 0, stream);
  return check_launch("step kernel");
}

// sample + step in one launch where the fused kernel exists (the drawn actions go to ge_buffers.actions_out when that is set),
// else two launches through `scratch`
static int sample_and_step(ge_engine *e, uint64_t policy_seed, int64_t *scratch, void *stream) {
  int rc = check_state(e);
  if (rc != GE_OK) return rc;
  if (dc_range(e)) {  // the coverage range kernel sits between the policy and the step
    if (!scratch) return fail(GE_E_BADARG, "this env type needs actions_scratch");
    rc = ge_sample_actions(e, policy_seed, scratch, stream);
    return rc == GE_OK ? ge_step_only(e, scratch, stream) : rc;
  }
  launch_step(e, true, nullptr, policy_seed, stream);
  return check_launch("fused sample+step kernel");
}

// regenerate the slots the most recent step launch queued
extern "C" int ge_reset_pending(ge_engine *e, void *stream) {
  if (!e) return fail(GE_E_BADARG, "null argument");
  int rc = check_state(e);
  if (rc != GE_OK) return rc;
  if (e->P.autoreset) {
    if (e->spares) {  // finished slots with a valid image: one streaming copy each
      int64_t grid = 1024;  // workgroups stride over (slot, part) items; most steps have a few hundred
      if (grid > (int64_t)e->P.B * e->swap_parts) grid = (int64_t)e->P.B * e->swap_parts;
      GE_LAUNCH(e->k.swap, (int)grid, 256, prefix_bytes(e->P.B), stream, e->P, e->R, e->RS, e->PS.buf, e->swap_parts);
      rc = check_launch("swap kernel");
      if (rc != GE_OK) return rc;
    }
    rc = launch_reset(e, e->P, e->R, nullptr, run_queue(e), kNoInject, e->spares, stream);  // (with spares: the slots that finished again before their image was refilled)
    if (rc == GE_OK && e->spares && ++e->pending_calls >= e->period) rc = refill_spares(e, stream);
  }
  return rc;
}

extern "C" int ge_step(ge_engine *e, const int64_t *actions, void *stream) {
  if (!e || !actions) return fail(GE_E_BADARG, "null argument");
  if (e->P.autoreset == 2) {  // next-step mode: the slots that finished in the previous step are regenerated first
    int rc = ge_reset_pending(e, stream);
    return rc == GE_OK ? ge_step_only(e, actions, stream) : rc;
  }
  int rc = ge_step_only(e, actions, stream);
  if (rc != GE_OK) return rc;
  return ge_reset_pending(e, stream);
}

// Checkpointing: the slabs are the whole state.  An engine whose slabs were restored from a snapshot of a reset engine holds an
// episode and a seeded generator ring.
extern "C" int ge_mark_restored(ge_engine *e) {
  if (!e) return GE_E_BADARG;
  e->loaded = true; e->seeded = true; e->streams = e->P.buf.stream_state != nullptr;
  e->pending_calls = e->period;  // (the caller restores or clears spare_state with the other slabs; refill at the next opportunity)
  return GE_OK;
}

extern "C" int ge_vectorize(ge_engine *e, float *out, void *stream) {
  if (!e || !out) return fail(GE_E_BADARG, "null argument");
  // multi-class engine: the classes' flat vectors follow one another, class after class
  const GeParams *first = e->n_classes > 0 ? e->classes.data() : &e->P;
  for (const GeParams *C = first; C < first + (e->n_classes > 0 ? e->n_classes : 1); C++) {
    const int64_t tot = (int64_t)C->B * obs_len(*C);
    int64_t blocks = (tot + 255) / 256; if (blocks > 256 * 32) blocks = 256 * 32;
    GE_LAUNCH(ge_k_vectorize, (int)blocks, 256, 0, stream, *C, out);
    int rc = check_launch("vectorize kernel");
    if (rc != GE_OK) return rc;
    out += tot;
  }
  return GE_OK;
}

extern "C" int ge_sample_actions(ge_engine *e, uint64_t policy_seed, int64_t *actions, void *stream) {
  if (!e || !actions) return fail(GE_E_BADARG, "null argument");
  int grid = (e->P.B + 255) / 256;
  GE_LAUNCH(e->k.sample, grid, 256, 0, stream, e->P, e->R, policy_seed, actions);
  return check_launch("sample kernel");
}

// ---- masked categorical policy head (ge_policy.h): the forward modes and the gradient kernel, launched here in one geometry
static int launch_policy_kernel(ge_engine *e, void (*kernel)(GeParams, GeRagged, GePolicyIO), const char *what, GePolicyIO io, void *stream) {
  io.group = e->plan.pol_group;
  GE_LAUNCH(kernel, e->plan.pol_grid, GE_POL_THREADS, 0, stream, e->P, e->R, io);
  return check_launch(what);
}
// the storage type and the scale of a policy call, before anything is launched
static int check_policy_input(int32_t dtype, float scale) {
  if (dtype < 0 || dtype >= GE_LOGITS_DTYPES) return fail(GE_E_BADARG, "logits_dtype is none of GE_LOGITS_F32, GE_LOGITS_BF16, GE_LOGITS_F16");
  if (!(scale > 0.0f) || !(scale <= 3.402823466e38f)) return fail(GE_E_BADARG, "the logits scale must be finite and > 0");
  return GE_OK;
}
static int launch_policy(ge_engine *e, int mode, int32_t dtype, GePolicyIO io, void *stream) {  // mode: GE_POL_SAMPLE / GREEDY / EVALUATE
  static_assert(GE_POL_GRAD >= GE_POL_MODES, "the gradient is no entry of policy_head");
  if (mode < 0 || mode >= GE_POL_MODES) return fail(GE_E_BADARG, "no such policy head mode");
  return launch_policy_kernel(e, e->k.policy_head[dtype][mode], "policy head kernel", io, stream);
}

extern "C" int ge_policy_sample_as(ge_engine *e, const void *logits, int32_t logits_dtype, float scale, uint64_t policy_seed, int32_t greedy,
                                   int64_t *actions, float *logp, float *entropy, void *stream) {
  if (!e || !logits || !actions) return fail(GE_E_BADARG, "null argument");
  int rc = check_policy_input(logits_dtype, scale);
  if (rc != GE_OK) return rc;
  if (!e->loaded) return fail(GE_E_STATE, "the engine holds no episode yet: call ge_reset (or ge_inject_state) first");
  GePolicyIO io = {};
  io.logits = logits; io.scale = scale; io.actions = actions; io.logp = logp; io.entropy = entropy; io.policy_seed = policy_seed;
  return launch_policy(e, greedy ? GE_POL_GREEDY : GE_POL_SAMPLE, logits_dtype, io, stream);
}

extern "C" int ge_policy_evaluate_as(ge_engine *e, const void *logits, int32_t logits_dtype, float scale, const uint8_t *mask,
                                     const int64_t *actions, float *logp, float *entropy, void *stream) {
  if (!e || !logits || !mask || !actions) return fail(GE_E_BADARG, "null argument");
  int rc = check_policy_input(logits_dtype, scale);
  if (rc != GE_OK) return rc;
  GePolicyIO io = {};
  io.logits = logits; io.scale = scale; io.mask = mask; io.given = actions; io.logp = logp; io.entropy = entropy;
  return launch_policy(e, GE_POL_EVALUATE, logits_dtype, io, stream);
}

extern "C" int ge_policy_backward_as(ge_engine *e, const void *logits, int32_t logits_dtype, float scale, const uint8_t *mask,
                                     const int64_t *actions, const float *grad_logp, const float *grad_entropy, void *grad_logits, void *stream) {
  if (!e || !logits || !mask || !actions || !grad_logits) return fail(GE_E_BADARG, "null argument");
  int rc = check_policy_input(logits_dtype, scale);
  if (rc != GE_OK) return rc;
  GePolicyIO io = {};
  io.logits = logits; io.scale = scale; io.mask = mask; io.given = actions;
  io.grad_logp = grad_logp; io.grad_entropy = grad_entropy; io.grad_logits = grad_logits;
  return launch_policy_kernel(e, e->k.policy_grad[logits_dtype], "policy gradient kernel", io, stream);
}

extern "C" int ge_policy_step_as(ge_engine *e, const void *logits, int32_t logits_dtype, float scale, uint64_t policy_seed, int32_t greedy,
                                 int64_t *actions, float *logp, float *entropy, void *stream) {
  if (!e || !logits || !actions) return fail(GE_E_BADARG, "null argument");
  int rc = check_state(e);  // (the guard of ge_step, before anything is launched; the sample call checks logits_dtype and scale)
  if (rc == GE_OK) rc = ge_policy_sample_as(e, logits, logits_dtype, scale, policy_seed, greedy, actions, logp, entropy, stream);
  return rc == GE_OK ? ge_step(e, actions, stream) : rc;
}

// the float32 entry points: the same calls with GE_LOGITS_F32 and scale 1.0f
extern "C" int ge_policy_sample(ge_engine *e, const float *logits, uint64_t policy_seed, int32_t greedy, int64_t *actions, float *logp,
                                float *entropy, void *stream) {
  return ge_policy_sample_as(e, logits, GE_LOGITS_F32, 1.0f, policy_seed, greedy, actions, logp, entropy, stream);
}
extern "C" int ge_policy_evaluate(ge_engine *e, const float *logits, const uint8_t *mask, const int64_t *actions, float *logp, float *entropy,
                                  void *stream) {
  return ge_policy_evaluate_as(e, logits, GE_LOGITS_F32, 1.0f, mask, actions, logp, entropy, stream);
}
extern "C" int ge_policy_backward(ge_engine *e, const float *logits, const uint8_t *mask, const int64_t *actions, const float *grad_logp,
                                  const float *grad_entropy, float *grad_logits, void *stream) {
  return ge_policy_backward_as(e, logits, GE_LOGITS_F32, 1.0f, mask, actions, grad_logp, grad_entropy, grad_logits, stream);
}
extern "C" int ge_policy_step(ge_engine *e, const float *logits, uint64_t policy_seed, int32_t greedy, int64_t *actions, float *logp,
                              float *entropy, void *stream) {
  return ge_policy_step_as(e, logits, GE_LOGITS_F32, 1.0f, policy_seed, greedy, actions, logp, entropy, stream);
}

extern "C" int ge_random_rollout(ge_engine *e, uint64_t policy_seed, int32_t n_steps, int64_t *scratch, void *stream) {
  if (!e) return fail(GE_E_BADARG, "null argument");
  for (int s = 0; s < n_steps; s++) {
    int rc = GE_OK;
    if (e->P.autoreset == 2) rc = ge_reset_pending(e, stream);
    if (rc == GE_OK) rc = sample_and_step(e, policy_seed, scratch, stream);
    if (rc == GE_OK && e->P.autoreset != 2) rc = ge_reset_pending(e, stream);
    if (rc != GE_OK) return rc;
  }
  return GE_OK;
}

// the timing events of the ge_timed_* calls, created at the first of them
static int ensure_events(ge_engine *e) {
  if (!e->have_events) { for (int k = 0; k < 4; k++) if (hipEventCreate(&e->ev[k]) != hipSuccess) return fail(GE_E_LAUNCH, "hipEventCreate failed"); e->have_events = true; }
  return GE_OK;
}

extern "C" int ge_timed_rollout(ge_engine *e, uint64_t policy_seed, int32_t n_steps, int64_t *scratch, void *stream,
                                double *step_ms, double *reset_ms, double *policy_ms) {
  if (!e || (!scratch && !path64(e))) return fail(GE_E_BADARG, "null argument");
  if (ensure_events(e) != GE_OK) return GE_E_LAUNCH;
  double ts = 0, tr = 0, tp = 0;
  hipStream_t st = (hipStream_t)stream;
  for (int s = 0; s < n_steps; s++) {
    int rc = GE_OK;
    if (e->P.autoreset == 2) rc = ge_reset_pending(e, stream);  // next-step mode: counted with nothing (the timed split is for same-step runs)
    (void)hipEventRecord(e->ev[0], st);
    if (rc == GE_OK && !path64(e)) rc = ge_sample_actions(e, policy_seed, scratch, stream);
    (void)hipEventRecord(e->ev[1], st);
    if (rc == GE_OK) rc = path64(e) ? sample_and_step(e, policy_seed, scratch, stream) : ge_step_only(e, scratch, stream);
    (void)hipEventRecord(e->ev[2], st);
    if (rc == GE_OK && e->P.autoreset != 2) rc = ge_reset_pending(e, stream);
    (void)hipEventRecord(e->ev[3], st);
    if (rc != GE_OK) return rc;
    if (hipEventSynchronize(e->ev[3]) != hipSuccess) return fail(GE_E_LAUNCH, "hipEventSynchronize failed");
    float a = 0, b = 0, c = 0;
    (void)hipEventElapsedTime(&a, e->ev[0], e->ev[1]); (void)hipEventElapsedTime(&b, e->ev[1], e->ev[2]); (void)hipEventElapsedTime(&c, e->ev[2], e->ev[3]);
    tp += a; ts += b; tr += c;
  }
  if (step_ms) *step_ms = ts;
  if (reset_ms) *reset_ms = tr;
  if (policy_ms) *policy_ms = tp;
  return GE_OK;
}

extern "C" int ge_timed_step_burst(ge_engine *e, uint64_t policy_seed, int32_t k, int64_t *scratch, void *stream, double *burst_ms) {
  if (!e || !burst_ms) return fail(GE_E_BADARG, "null argument");
  if (ensure_events(e) != GE_OK) return GE_E_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  (void)hipEventRecord(e->ev[0], st);
  for (int j = 0; j < k; j++) { int rc = sample_and_step(e, policy_seed, scratch, stream); if (rc != GE_OK) return rc; }
  (void)hipEventRecord(e->ev[1], st);
  if (hipEventSynchronize(e->ev[1]) != hipSuccess) return fail(GE_E_LAUNCH, "hipEventSynchronize failed");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
  *burst_ms = ms;
  return GE_OK;
}

// the launch floor of the step kernel's shape (bench.py: reported beside the kernel's own duration, never subtracted from it)
GE_KERNEL ge_k_empty(int) {}
extern "C" int ge_timed_empty_burst(ge_engine *e, int32_t k, void *stream, double *burst_ms) {
  if (!e || !burst_ms) return fail(GE_E_BADARG, "null argument");
  if (ensure_events(e) != GE_OK) return GE_E_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  (void)hipEventRecord(e->ev[0], st);
  for (int j = 0; j < k; j++) GE_LAUNCH(ge_k_empty, step_blocks(e->P.B), e->k.step_threads, e->k.step_lds, stream, 0);
  (void)hipEventRecord(e->ev[1], st);
  if (hipEventSynchronize(e->ev[1]) != hipSuccess) return fail(GE_E_LAUNCH, "hipEventSynchronize failed");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
  *burst_ms = ms;
  return check_launch("empty kernel");
}

#if !defined(GE_EMU)
// diagnostic (tools/occupancy.py): resident workgroups per CU the runtime reports for the reset-path kernels
extern "C" int ge_debug_occupancy(ge_engine *e, int *out4) {
  if (!e || !out4) return GE_E_BADARG;
  int a = -1, b = -1, c = -1, d = -1;
  const GePlan &L = e->plan;
  const GeBucket *K = L.bk;  // the engine's first bucket
  while (!K->used) K++;
  const void *step = path64(e) ? (const void *)e->k.step_path64[1][e->spares] : (const void *)e->k.step[1];
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, (const void *)e->k.reset, GE_RESET_THREADS, K->graph.lds);
  if (L.feat_fast) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void *)e->k.features64, GE_F64_THREADS, L.f64_lds);
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&c, (const void *)e->k.features, K->gen.threads, K->gen.lds);
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&d, step, e->k.step_threads, e->k.step_lds);
  out4[0] = a; out4[1] = b; out4[2] = c; out4[3] = d;
  return GE_OK;
}
#endif

#if defined(GE_STAMPS) && !defined(GE_EMU)
// diagnostic build only: copy out the phase timestamps of slot 0 (synchronises)
extern "C" int ge_debug_read_stamps(unsigned long long *out32) {
  return hipMemcpyFromSymbol(out32, HIP_SYMBOL(ge_stamp_buf), 32 * sizeof(unsigned long long)) == hipSuccess ? GE_OK : GE_E_LAUNCH;
}
#endif
