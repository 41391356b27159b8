// Masked categorical policy head: logits in, {action, log-probability, entropy} of every slot out in ONE launch
// (ge_policy_sample / ge_policy_evaluate / ge_policy_step, include/graphenvs.h).  Replaces, for a caller of the reference, the
// masked_fill(~info['mask']) -> log_softmax -> sample -> gather -> entropy chain between the network and env.step().
//
// Arithmetic of a row (float32): mx = max of the valid logits, d = l - mx, w = expf(d) for valid actions and 0
// otherwise, Z = sum w, logp[a] = d[a] - logf(Z), entropy = logf(Z) - (sum w d) / Z.  A row is worked on by one lane GROUP and
// by nothing else: `group` lanes (a power of two, the same for every row of the launch), element j * group + g of the row in
// lane g at chunk j.  Every sum is a fixed tree over (chunk, lane), so a row's result depends on the row alone -- not on the
// batch size, the slot's place in the launch or its neighbours.
//  - rows of at most 64 actions: group = the power of two covering the widest row, 64 / group rows per wave, one chunk;
//  - longer rows: group = 64, a wave per row, coalesced chunks of 64.  Up to GE_POL_REG_CHUNKS chunks (2 048 actions, BASELINE
//    config 4's row) the row is loaded ONCE and stays in registers between the max / sum pass and the prefix pass (expf is
//    recomputed, w is not kept); a longer row is read twice: pass 1 keeps a running maximum and a sum rescaled under it per
//    lane, pass 2 is the prefix pass.
// Validity comes from the engine's mask_bits (sample, greedy: chunk j of a wave-wide row IS word j of the mask row; the [B, A]
// bool slab is never read) or from the caller's bool bytes at the logits' own indices (evaluate, gradient).
//
// Gradient (ge_policy_backward, ge_k_policy_grad): the same row pass -- ge_pol_rows, the body of both kernels -- in the geometry of
// the forward, then, with p = w / Z, lp = d - logf(Z), H the entropy and the upstream gradients gl (of logp) and gh (of entropy),
//   grad[a] = gl ([a == a*] - p[a]) - gh p[a] (lp[a] + H)  for a valid a,  0.0 for a masked one;
// gl counts as 0 where the action a* is -1, out of range or masked out (the forward's logp is -inf there).  A row held in registers
// is stored from them, chunk after chunk (4 B of logit and 1 B of mask read, 4 B written per element); a longer row is read a
// third time.  Every element of every row is written; lanes and chunks past the row's end store nothing.
//
// Storage type and scale (the *_as entry points; ge_policy_sample and its kin are float32 with scale 1.0f).  The logits are float32,
// bfloat16 or float16 words, the kernels are instantiated per type.  An element is converted to float32 (exact) and multiplied by
// io.scale, the product rounded to float32 ONCE: that product is l everywhere above -- mx, d, w, Z, the prefix sums, the greedy
// comparison and the writer lane's re-read of x[a] -- so a 16-bit launch equals the float32 launch on float(x) * scale bit for bit
// (x 1.0f is exact: the float32 path with scale 1 computes what it did before the scale existed).  The gradient is stored in the
// logits' type: round_to_nearest_even(g * scale), g the float32 gradient above, a masked element +0.0 (a VALID element whose gradient
// is zero may carry either sign, as in float32: the row with one valid action gets gl * (1 - 1), -0.0 for gl < 0).  One load helper and one store
// helper (ge_pol_load / ge_pol_store) are the only places that know the type; the (chunk, lane) mapping and every tree are the
// float32 kernel's.  16-bit rows start at element i * A, 2-byte aligned only: every lane loads and stores single 2-byte words
// (2 B of logit and 1 B of mask read, 2 B written per element).
#pragma once
#include <math.h>

#include "ge_params.h"
#include "ge_platform.h"
#include "ge_step.h"

// forward modes (the GE_POL_MODES entries of GeKernels.policy_head), then the gradient: ge_k_policy_grad, no entry of that table
enum { GE_POL_SAMPLE = 0, GE_POL_GREEDY = 1, GE_POL_EVALUATE = 2, GE_POL_MODES = 3, GE_POL_GRAD = 3 };
#define GE_POL_THREADS 256
#define GE_POL_REG_CHUNKS 32  // chunks of a row held in registers: 64 * 32 = 2 048 actions
#define GE_POL_BLOCK 8        // chunks a longer row loads back to back
template <int N> struct GeInt { static constexpr int value = N; };

struct GePolicyIO {
  const void *logits;     // the classes' [B_c, A_c] blocks one after the other (GeParams.policy_off), in the kernel's storage type
  const uint8_t *mask;    // evaluate, gradient: bool bytes in the layout of logits
  const int64_t *given;   // evaluate, gradient: the actions to score
  int64_t *actions;       // sample, greedy
  float *logp, *entropy;  // may be NULL
  uint64_t policy_seed;
  int32_t group;          // lanes per row (GePlan.pol_group)
  const float *grad_logp, *grad_entropy;  // gradient: upstream [B] of logp and entropy, NULL: zeros
  void *grad_logits;                      // gradient: out, in the layout and the storage type of logits
  float scale;                            // every element times this, in float32, is "the logit" (1.0f: the element itself)
};

// THE load and THE store of the logits' storage type T (float, ge_bf16, ge_f16: ge_platform.h).  Load: the element as float32 (exact,
// ge_pol_raw) times scale, ONE float32 rounding (ge_pol_scaled) -- the logit of everything below; ge_pol_load is the two together,
// for a single element.  Where several elements are loaded back to back (the chunks of a row in registers, the blocks of a longer
// row) the place of the multiplies is chosen per kernel, by measurement (MI355X, against the kernel without a scale):
//  - evaluate, row in registers: the ge_pol_raw loads first, each ge_pol_scaled in the loop that first uses the elements, behind the
//    chunk's validity bit.  The in-place multiply is an asm statement and the compiler keeps it where the source has it.  Inside
//    the load loop it sat between the loads with an s_waitcnt vmcnt(0) in front, and a row of two chunks made two memory round trips
//    instead of one (18.6 us instead of 16.8 for three classes of 12 / 64 / 100 actions, 48.4 instead of 46.4 at 2 048 actions).
//    In a loop of its own behind the loads the kernel takes 116 VGPRs, in front of the validity bit 80 / 82, behind it the 78 / 80
//    of the kernel without a scale;
//  - sample, greedy: inside the load loop.  Their validity loop holds a ds_bpermute per chunk, and an asm statement between them
//    keeps the compiler from issuing those back to back (2 048 actions: 99.2 us instead of 93.2); their loads carry no mask bytes;
//  - gradient: inside the load loop, as a plain multiply (in-place: 108 us instead of 80 at 2 048 actions);
//  - a block of a longer row: eight loads, then eight multiplies.
// Store: the gradient with respect to that logit times scale (one float32 multiply), rounded to T to nearest even.
// The multiply of the forward kernels is ge_mul_f32_inplace (ge_platform.h): one v_mul_f32 whose product lands in the register the
// element was loaded into (profiles/r05_policy_dtype.txt):
//  - written as `* scale` the float32 evaluate kernel took 89 VGPRs (91 for a multi-class engine) instead of the 78 / 80 it has without
//    a scale, five waves per SIMD instead of six, and 37.0 us instead of 33.2 at 65 536 rows of 64 actions;
template <class T> GE_DEV float ge_pol_raw(const T *x, int64_t k) { return ge_to_f32(x[k]); }
template <int MODE> GE_DEV float ge_pol_scaled(float raw, float scale) { return MODE == GE_POL_GRAD ? raw * scale : ge_mul_f32_inplace(raw, scale); }
template <int MODE, class T> GE_DEV float ge_pol_load(const T *x, int64_t k, float scale) { return ge_pol_scaled<MODE>(ge_pol_raw(x, k), scale); }
template <class T> GE_DEV void ge_pol_store(T *out, int64_t k, float g, float scale) { out[k] = ge_from_f32(g * scale, T()); }

// lane group of a row: lanes [lane - g, lane - g + G), G a power of two.  Every lane of the group executes these.
GE_DEV float ge_shfl_f32(float v, int src) {
  uint32_t u; __builtin_memcpy(&u, &v, 4);
  u = ge_shfl_u32(u, src);
  __builtin_memcpy(&v, &u, 4);
  return v;
}
GE_DEV float ge_grp_max(float v, int lane, int G) { for (int o = G >> 1; o; o >>= 1) v = fmaxf(v, ge_shfl_f32(v, lane ^ o)); return v; }
GE_DEV int ge_grp_max_i32(int v, int lane, int G) { for (int o = G >> 1; o; o >>= 1) { const int t = ge_shfl_i32(v, lane ^ o); v = t > v ? t : v; } return v; }
// (a + b == b + a bit for bit: every lane of the group ends with the same sum)
GE_DEV float ge_grp_sum(float v, int lane, int G) { for (int o = G >> 1; o; o >>= 1) v += ge_shfl_f32(v, lane ^ o); return v; }
// inclusive prefix over the lanes of the group
GE_DEV float ge_grp_prefix(float v, int lane, int G) {
  const int g = lane & (G - 1);
  for (int o = 1; o < G; o <<= 1) { const float t = ge_shfl_f32(v, g >= o ? lane - o : lane); if (g >= o) v += t; }
  return v;
}
// the group's lanes of a ballot, lane g of the group in bit g
GE_DEV uint64_t ge_grp_ballot(bool p, int lane, int G) {
  const uint64_t b = ge_ballot(p) >> (lane & ~(G - 1));
  return G == 64 ? b : (b & ((1ull << G) - 1ull));
}

// One chunk of the prefix pass.  xj / v: this lane's logit and its validity; mx, t: the row's maximum and u * Z.
// s1 gathers w * d; act (-1: not found yet) the sampled / greedy action, carry the prefix in front of the chunk.
template <int MODE>
GE_DEV void ge_pol_chunk(float xj, bool v, int first, float mx, float t, int lane, int G, float &s1, float &carry, int &act) {
  const float d = v ? xj - mx : 0.0f, w = v ? expf(d) : 0.0f;
  s1 += w * d;
  if (MODE == GE_POL_EVALUATE || MODE == GE_POL_GRAD || act >= 0) return;  // (act is the same in every lane of the group)
  if (MODE == GE_POL_GREEDY) {
    const uint64_t hit = ge_grp_ballot(v && xj == mx, lane, G);
    if (hit) act = first + ge_ctz64(hit);
    return;
  }
  const float p = carry + ge_grp_prefix(w, lane, G);
  const uint64_t hit = ge_grp_ballot(v && p > t, lane, G);
  if (hit) act = first + ge_ctz64(hit);
  else carry = ge_shfl_f32(p, (lane | (G - 1)));
}

// the row's entropy from its gathered s1 and Z; lz = logf(Z).  Every lane of the group executes this.
GE_DEV float ge_pol_entropy(float s1, float Z, int lane, int G, float &lz) {
  const float S1 = ge_grp_sum(s1, lane, G);
  lz = logf(Z);
  return lz - S1 / Z;
}

// what the gradient of a row's elements shares: a row without a valid action keeps the zeros (none of its elements is valid)
struct GePolGradRow { float mx, lz, rZ, H, gl, gh; int astar; };
GE_DEV float ge_pol_grad_at(const GePolGradRow &c, float xj, bool v, int idx) {
  const float d = v ? xj - c.mx : 0.0f, p = expf(d) * c.rZ, lp = d - c.lz;
  const float gr = c.gl * ((idx == c.astar ? 1.0f : 0.0f) - p) - c.gh * (p * (lp + c.H));
  return v ? gr : 0.0f;
}

// The body of ge_k_policy_head<RAGGED, MODE> and, with MODE = GE_POL_GRAD, of ge_k_policy_grad<RAGGED>.
template <bool RAGGED, int MODE, class T>
GE_DEV void ge_pol_rows(const GeParams &PG, const GeRagged &R, const GePolicyIO &io) {
  constexpr bool EVAL = MODE == GE_POL_EVALUATE || MODE == GE_POL_GRAD;  // validity from the caller's bytes, nothing of the episode read
  const int tid = ge_tid(), lane = tid & 63;
  const int G = io.group, g = lane & (G - 1), gbase = lane - g;
  const int64_t item = (int64_t)ge_bid() * (GE_POL_THREADS / 64) + (tid >> 6);  // this wave's 64 / G rows
  const int64_t slot = item * (64 / G) + (lane - g) / G;
  if (slot >= PG.B) return;  // (whole groups leave: a group never straddles rows)
  const int ig = (int)slot;
  int cls = 0, lo = 0;
  if constexpr (RAGGED) {
    cls = R.slot_class[ig];
    if (G == 64) cls = (int)ge_uniform_u32((uint32_t)cls);
    lo = R.class_start[cls];
  }
  const GeParams &P = RAGGED ? R.classes[cls] : PG;
  const int i = ig - lo, A = P.A, AW = P.AW;
  const int64_t row = P.policy_off + (int64_t)i * A;
  const T *x = (const T *)io.logits + row;
  const float scale = io.scale;
  const uint8_t *mbytes = EVAL ? io.mask + row : nullptr;
  const uint64_t *mb = P.buf.mask_bits + (int64_t)i * AW;
  const int nch = G < 64 ? 1 : (A + 63) >> 6;  // (G < 64: every row of the launch fits its group)
  // mask words j0 .. j0 + G - 1 of the row, word j0 + g in lane g: one unconditional load (a word past the end re-reads word 0)
  auto words_at = [&](int j0) { return mb[j0 + g < AW ? j0 + g : 0]; };
  const bool writer = g == 0;
  uint64_t packed = 0;
  if (!EVAL) packed = P.buf.slot_rec[2 * (int64_t)i + 1];

  float mx = -INFINITY, Z = 0.0f, s1 = 0.0f, carry = 0.0f, t = 0.0f;
  int act = -1, last = -1;  // last: the highest valid action of this lane
  bool any;
  auto threshold = [&]() {  // the draw of this slot and step: the key of ge_policy_draw
    const uint64_t z = ge_mix64(io.policy_seed + (uint64_t)(P.env_index_base + i) * 0x9E3779B97F4A7C15ull + ge_rec_tstep(packed) * 0xD1B54A32D192ED03ull);
    return ((float)(z >> 40) * 0x1p-24f) * Z;
  };
  const bool frozen = !EVAL && ge_policy_idle(1u, ge_rec_status(packed));
  // gradient: the row's action and upstream gradients, asked for in front of the row (every lane of the group: one address each)
  GePolGradRow gr = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1};
  if (MODE == GE_POL_GRAD) {
    const int64_t a = io.given[ig];
    const bool ok = a >= 0 && a < (int64_t)A && mbytes[a] != 0;  // else the forward's logp is -inf: its gradient is dropped
    if (ok) gr.astar = (int)a;
    if (ok && io.grad_logp) gr.gl = io.grad_logp[ig];
    if (io.grad_entropy) gr.gh = io.grad_entropy[ig];
  }
  T *gout = MODE == GE_POL_GRAD ? (T *)io.grad_logits + row : nullptr;
  auto grad_row = [&]() {  // after the row pass (any, mx, Z, s1)
    if (!any) return;
    gr.mx = mx; gr.rZ = 1.0f / Z;
    gr.H = ge_pol_entropy(s1, Z, lane, G, gr.lz);
  };
  // ---- the row in registers.  NCH, the row's chunk count rounded up to a power of two, is a compile-time constant: the loops
  // unroll fully, xv[] is indexed statically and the NCH loads (a chunk past the row re-reads element 0) are issued back to back
  // in front of the first use.
  auto in_regs = [&](auto nc) {
    constexpr int NCH = decltype(nc)::value;
    constexpr bool LATE = MODE == GE_POL_EVALUATE;  // where the multiply of the row's elements stands (ge_pol_scaled, above)
    float xv[NCH];
    uint8_t mv[NCH];
    uint32_t vb = 0;  // bit j: element j * G + g is a valid action
    uint64_t words = 0;
    if (!EVAL) words = words_at(0);
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const int idx = j * G + g;
      xv[j] = LATE ? ge_pol_raw(x, idx < A ? idx : 0) : ge_pol_load<MODE>(x, idx < A ? idx : 0, scale);
      if (EVAL) mv[j] = mbytes[idx < A ? idx : 0];
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const int idx = j * G + g;
      bool v;  // (every lane of the group takes part in the shuffle, also one past the row's end)
      if (EVAL) v = idx < A && mv[j] != 0;
      else { const uint64_t mw = ge_shfl_u64(words, gbase + j); v = idx < A && ((mw >> (idx & 63)) & 1ull) != 0ull; }
      vb |= (uint32_t)v << j;
      if (LATE) xv[j] = ge_pol_scaled<MODE>(xv[j], scale);  // (from here on xv[j] is the logit: every use below comes after this loop)
      if (v) m = fmaxf(m, xv[j]);
    }
    mx = ge_grp_max(m, lane, G);
    any = ge_grp_ballot(vb != 0u, lane, G) != 0ull;
    if (any && !frozen) {
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < NCH; j++)
        if ((vb >> j) & 1u) s += expf(xv[j] - mx);
      Z = ge_grp_sum(s, lane, G);
      if (MODE == GE_POL_SAMPLE) t = threshold();
#pragma unroll
      for (int j = 0; j < NCH; j++)
        if (j < nch) ge_pol_chunk<MODE>(xv[j], ((vb >> j) & 1u) != 0u, j * G, mx, t, lane, G, s1, carry, act);
      if (vb) last = (31 - ge_clz32(vb)) * G + g;
    }
    if (MODE == GE_POL_GRAD) {  // the gradient from the registers: NCH values, then their stores back to back
      grad_row();
      float gv[NCH];
#pragma unroll
      for (int j = 0; j < NCH; j++) gv[j] = ge_pol_grad_at(gr, xv[j], ((vb >> j) & 1u) != 0u, j * G + g);
      // a row of more than NCH / 2 chunks of 64 lanes (every row the dispatch below hands an NCH >= 2) holds its first NCH / 2 chunks
      // whole: every lane stores them, without a test
      constexpr int HALF = NCH / 2;
      if (G == 64 && nch > HALF) {
#pragma unroll
        for (int j = 0; j < HALF; j++) ge_pol_store(gout, j * 64 + g, gv[j], scale);
#pragma unroll
        for (int j = HALF; j < NCH; j++)
          if (j * 64 + g < A) ge_pol_store(gout, j * 64 + g, gv[j], scale);
      } else {
#pragma unroll
        for (int j = 0; j < NCH; j++)
          if (j * G + g < A) ge_pol_store(gout, j * G + g, gv[j], scale);
      }
    }
  };
  if (nch <= 1) in_regs(GeInt<1>());
  else if (nch <= 2) in_regs(GeInt<2>());
  else if (nch <= 4) in_regs(GeInt<4>());
  else if (nch <= 8) in_regs(GeInt<8>());
  else if (nch <= 16) in_regs(GeInt<16>());
  else if (nch <= GE_POL_REG_CHUNKS) in_regs(GeInt<GE_POL_REG_CHUNKS>());
  else {
    // ---- a row above 2 048 actions (a wave per row): read twice, GE_POL_BLOCK chunks loaded back to back at a time
    float m = -INFINITY, s = 0.0f;
    uint64_t words = 0;
    bool seen = false;
    float xs[GE_POL_BLOCK];
    uint8_t ms[GE_POL_BLOCK];
    auto load_block = [&](int j0) {  // (a chunk past the row re-reads element 0 and counts as invalid)
      if (!EVAL && (j0 & 63) == 0) words = words_at(j0);
#pragma unroll
      for (int k = 0; k < GE_POL_BLOCK; k++) {
        const int idx = (j0 + k) * 64 + lane;
        xs[k] = ge_pol_raw(x, idx < A ? idx : 0);
        if (EVAL) ms[k] = mbytes[idx < A ? idx : 0];
      }
#pragma unroll
      for (int k = 0; k < GE_POL_BLOCK; k++) xs[k] = ge_pol_scaled<MODE>(xs[k], scale);
    };
    auto valid_at = [&](int j0, int k) {
      const int idx = (j0 + k) * 64 + lane;
      if (EVAL) return idx < A && ms[k] != 0;
      const uint64_t mw = ge_shfl_u64(words, (j0 + k) & 63);  // (every lane takes part, also one past the row's end)
      return idx < A && ((mw >> (idx & 63)) & 1ull) != 0ull;
    };
    for (int j0 = 0; j0 < nch; j0 += GE_POL_BLOCK) {
      load_block(j0);
#pragma unroll
      for (int k = 0; k < GE_POL_BLOCK; k++) {
        const float xj = xs[k];
        if (valid_at(j0, k)) {
          if (xj > m) { s = s * expf(m - xj) + 1.0f; m = xj; }  // (first element: 0 * expf(-inf) + 1)
          else s += expf(xj - m);
          seen = true; last = (j0 + k) * 64 + lane;
        }
      }
    }
    mx = ge_grp_max(m, lane, G);
    any = ge_grp_ballot(seen, lane, G) != 0ull;
    if (any && !frozen) {
      Z = ge_grp_sum(seen ? s * expf(m - mx) : 0.0f, lane, G);
      if (MODE == GE_POL_SAMPLE) t = threshold();
      for (int j0 = 0; j0 < nch; j0 += GE_POL_BLOCK) {
        load_block(j0);
#pragma unroll
        for (int k = 0; k < GE_POL_BLOCK; k++)
          if (j0 + k < nch) ge_pol_chunk<MODE>(xs[k], valid_at(j0, k), (j0 + k) * 64, mx, t, lane, G, s1, carry, act);
      }
    }
    if (MODE == GE_POL_GRAD) {  // a third read of the row
      grad_row();
      for (int j0 = 0; j0 < nch; j0 += GE_POL_BLOCK) {
        load_block(j0);
        float gv[GE_POL_BLOCK];
#pragma unroll
        for (int k = 0; k < GE_POL_BLOCK; k++) gv[k] = ge_pol_grad_at(gr, xs[k], valid_at(j0, k), (j0 + k) * 64 + lane);
#pragma unroll
        for (int k = 0; k < GE_POL_BLOCK; k++)
          if ((j0 + k) * 64 + lane < A) ge_pol_store(gout, (j0 + k) * 64 + lane, gv[k], scale);
      }
    }
  }
  if (MODE == GE_POL_GRAD) return;
  const bool idle = !any || frozen;
  float lp = 0.0f, ent = 0.0f;
  if (!idle) {
    float lz;
    ent = ge_pol_entropy(s1, Z, lane, G, lz);
    // rounding left no prefix above t: the last valid action (greedy: only non-finite logits get here; x[act] stays inside the row)
    if (MODE != GE_POL_EVALUATE && act < 0) act = ge_grp_max_i32(last, lane, G);
  }
  if (!writer) return;
  if (MODE == GE_POL_EVALUATE) {
    const int64_t a = io.given[ig];
    const bool ok = !idle && a >= 0 && a < (int64_t)A && mbytes[a] != 0;
    lp = ok ? (ge_pol_load<MODE>(x, a, scale) - mx) - logf(Z) : -INFINITY;  // (ok: a is inside the row)
  } else {
    if (!idle) lp = (ge_pol_load<MODE>(x, act, scale) - mx) - logf(Z);
    io.actions[ig] = idle ? -1 : (int64_t)act;
  }
  if (io.logp) io.logp[ig] = lp;
  if (io.entropy) io.entropy[ig] = ent;
}

template <bool RAGGED, int MODE, class T>
GE_KERNEL_LB(GE_POL_THREADS, 1) ge_k_policy_head(GeParams PG, GeRagged R, GePolicyIO io) { ge_pol_rows<RAGGED, MODE, T>(PG, R, io); }

template <bool RAGGED, class T>
GE_KERNEL_LB(GE_POL_THREADS, 1) ge_k_policy_grad(GeParams PG, GeRagged R, GePolicyIO io) { ge_pol_rows<RAGGED, GE_POL_GRAD, T>(PG, R, io); }
