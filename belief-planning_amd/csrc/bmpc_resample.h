// bmpc_resample.h -- resampling a weighted closed-loop population (bmpc_population_ancestors,
// bmpc_gather_egos, bmpc_resample_device): the per-element rules, the same text on host and device.
//
// The ancestor rule is defined on integers, so that a parallel scan of any shape, a g++ build and
// bmpc/resample.py all give the same ancestors:
//   M   = max_i logw_i                        (M = -inf: nothing is resampled)
//   k_i = floor(exp(logw_i - M) 2^40)         uint64; logw = -inf gives 0
//   C_i = k_0 + ... + k_i,  S = C_{B-1}       B <= 2^20, so S < 2^61
//   Q   = sum k_i^2                           exact in 128 bits
//   ess = (double)S (double)S / (double)Q     conversions round to nearest, as Python's float(int)
//   u53 = the 53-bit numerator of rng_uniform53 of Philox4x32-10 at counter
//         {lo32(ego_base), hi32(ego_base), round, purpose 1}, key = seed;  U0 = (u53 S) >> 53 < S
// Systematic resampling: child j's raw ancestor is the smallest i with C_i B > U0 + j S (128-bit
// products, no division); n_i children have raw ancestor i.  Arrangement: survivors stay where they
// are -- a slot with n_i >= 1 keeps ancestor[i] = i, and the dead slots (n_i = 0), in increasing
// order, receive the surplus list (each i repeated n_i - 1 times, in increasing i).  Sources are
// therefore never destinations.  Every ego's new log-weight is M + log S - log B - 40 log 2, the log
// of the mean weight.
#pragma once

#include "bmpc_rng.h"

namespace bmpc {

typedef unsigned __int128 u128;

enum { RNG_PURPOSE_RESAMPLE = 1 };   // counter word 3 of the resampling draw (bmpc_rng.h reserves it)
enum { RESAMPLE_BITS = 40, RESAMPLE_MAX_BATCH = 1 << 20 };

// a log-weight that refuses the resampling: NaN or +inf (-inf is a dead ego, weight 0)
BMPC_HD bool resample_bad_logw(double lw) { return lw != lw || lw == INFINITY; }

// k = floor(exp(logw - M) 2^40) for a finite M >= logw
BMPC_HD uint64_t resample_quantise(double logw, double M) {
  if (!(logw > -INFINITY)) return 0;
  return (uint64_t)floor(exp(logw - M) * 1099511627776.0);
}

// the 53-bit integer of the one draw of a resampling
BMPC_HD uint64_t resample_u53(uint64_t seed, uint64_t ego_base, uint32_t round) {
  const uint32_t c[4] = {(uint32_t)ego_base, (uint32_t)(ego_base >> 32), round, RNG_PURPOSE_RESAMPLE};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t o[4];
  philox4x32_10(c, k, o);
  return ((uint64_t)(o[0] >> 5) << 26) | (uint64_t)(o[1] >> 6);
}

// U0 = (u53 S) >> 53, in [0, S)
BMPC_HD u128 resample_offset(uint64_t u53, uint64_t S) { return ((u128)u53 * S) >> 53; }

// (double)v, rounded to nearest (ties to even): Python's float(int).  Written out because the
// device has no 128-bit conversion: the top 64 bits with a sticky bit below them, then one hardware
// conversion (the sticky bit sits 10 places below the rounding position).
BMPC_HD double resample_to_double(u128 v) {
  const uint64_t hi = (uint64_t)(v >> 64), lo = (uint64_t)v;
  if (hi == 0) return (double)lo;
  int nb = 1;
  while (nb < 64 && (hi >> nb) != 0) ++nb;   // hi has nb significant bits: top = v >> nb
  const uint64_t top = nb < 64 ? (hi << (64 - nb)) | (lo >> nb) : hi;
  const bool sticky = nb < 64 ? (lo << (64 - nb)) != 0 : lo != 0;
  return ldexp((double)(top | (sticky ? 1 : 0)), nb);
}

BMPC_HD double resample_ess(uint64_t S, u128 Q) {
  const double s = (double)S;
  return s * s / resample_to_double(Q);
}

// the log of the mean weight: every ego's log-weight after a resampling
BMPC_HD double resample_new_logw(double M, uint64_t S, int B) {
  return M + log((double)S) - log((double)B) - 40.0 * log(2.0);
}

// the number of children j in [0, B) with U0 + j S < c B: the children whose raw ancestor lies at or
// before the slot whose inclusive prefix sum is c.  n_i = below(C_i) - below(C_{i-1}).
BMPC_HD int resample_children_below(uint64_t c, uint64_t S, u128 U0, int B) {
  const u128 lim = (u128)c * (uint64_t)B;
  int lo = 0, hi = B;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (U0 + (u128)(uint64_t)mid * S < lim) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// child j's raw ancestor: the smallest i with C_i B > U0 + j S (C the inclusive prefix sums)
BMPC_HD int resample_raw_ancestor(const uint64_t* C, int B, uint64_t S, u128 U0, int j) {
  const u128 thr = U0 + (u128)(uint64_t)j * S;
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((u128)C[mid] * (uint64_t)B > thr) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The arrangement works on one scan: slot i contributes (dead, surplus) = (n_i == 0, max(n_i - 1, 0))
// packed as dead << 32 | surplus (both sums are at most B <= 2^20), P the inclusive prefix sums.
BMPC_HD uint64_t resample_pack(int n) { return n == 0 ? (uint64_t)1 << 32 : (uint64_t)(n - 1); }

// ancestor[i] from P: a surviving slot keeps itself; the dead slot of rank r (counting from 0) takes
// entry r of the surplus list, i.e. the smallest i' whose inclusive surplus sum exceeds r.
BMPC_HD int resample_arrange(const uint64_t* P, int B, int i) {
  const uint32_t dead_incl = (uint32_t)(P[i] >> 32), dead_before = i ? (uint32_t)(P[i - 1] >> 32) : 0;
  if (dead_incl == dead_before) return i;
  const uint32_t r = dead_before;
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((uint32_t)P[mid] > r) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------
// What an ego is, besides its rows in the caller's buffers and its policy row: the spans of its
// workspace slab that a later solve or scene step reads before writing them (offsets and lengths
// in doubles).  The tree update reads uLin, pprev and misc (MISC_INIT, MISC_JCONS, MISC_OLDU,
// MISC_BEST, MISC_X0); write_outputs, the recorder and the fused loops read xpred, upred and sol;
// robustMPC's tree reads xlin; transform and merge plans keep S / bx / Fx, their flags and the
// state rows in xform.  Everything else in the slab is written by a solve before that solve reads
// it (the tree of the current solve, the IPM's and the QP's vectors, the small-batch kernel's
// LDS-resident spans).
// ------------------------------------------------------------------------------------------------
struct EgoSpan {
  size_t off, len;
};
enum { EGO_MAX_SPANS = 8 };

BMPC_HD int ego_state_spans(const Plan& P, const Layout& L, EgoSpan* out) {
  int k = 0;
  out[k++] = EgoSpan{L.uLin, (size_t)(P.U + 1) * P.d};
  out[k++] = EgoSpan{L.pprev, (size_t)P.bdim * P.m};
  out[k++] = EgoSpan{L.misc, (size_t)(8 + BMPC_MAX_N)};
  out[k++] = EgoSpan{L.xpred, (size_t)P.T * P.n};
  out[k++] = EgoSpan{L.upred, (size_t)P.U * P.d};
  out[k++] = EgoSpan{L.sol, (size_t)P.nv};
  if (P.desc.controller == BMPC_CTRL_ROBUST) out[k++] = EgoSpan{L.xlin, (size_t)P.T * P.n};
  if (P.desc.model == BMPC_MODEL_HIGHWAY_MERGE ||
      (P.desc.model == BMPC_MODEL_HIGHWAY && (P.desc.flags & BMPC_PLAN_TRANSFORM)))
    out[k++] = EgoSpan{L.xform, (size_t)XF_COUNT};
  return k;
}

// ------------------------------------------------------------------------------------------------
// The gather "ego j continues as a copy of ego a[j]": a list of row segments (a base, the bytes
// between egos, the segment's offset in an ego's row and its length, all in 4-byte words so that
// the int32 columns ride along), staged through a scratch row per ego and committed by a second
// pass, so that any map -- a permutation, a broadcast -- copies the egos as they were before.
// ------------------------------------------------------------------------------------------------
struct GatherSeg {
  uint32_t* base;    // ego 0's row
  size_t stride;     // words between egos
  size_t off;        // the segment's first word in a row
  uint32_t words;    // its length
  uint32_t at;       // its first word in the ego's staging row
};
enum { GATHER_MAX_SEGS = 24 };
struct GatherList {
  GatherSeg seg[GATHER_MAX_SEGS];
  int nseg;
  int batch;
  uint32_t row_words;   // words of one staging row
};

BMPC_HD bool gather_add(GatherList& G, void* base, size_t stride_words, size_t off_words, size_t words) {
  if (!base || words == 0) return true;
  if (G.nseg >= GATHER_MAX_SEGS) return false;
  G.seg[G.nseg++] = GatherSeg{(uint32_t*)base, stride_words, off_words, (uint32_t)words, G.row_words};
  G.row_words += (uint32_t)words;
  return true;
}

// a[j] clamped to an ego of the batch (as the script column is clamped to a policy)
BMPC_HD int gather_source(const int32_t* anc, int batch, int j) {
  const int a = anc[j];
  return a < 0 ? 0 : a >= batch ? batch - 1 : a;
}

// pass 1, ego j (lanes lane, lane + nlanes, ...): its source's segments into staging row j
BMPC_HD void gather_stage_ego(const GatherList& G, const int32_t* anc, uint32_t* stage, int j, int lane, int nlanes) {
  const int a = gather_source(anc, G.batch, j);
  if (a == j) return;
  uint32_t* row = stage + (size_t)j * G.row_words;
  for (int s = 0; s < G.nseg; ++s) {
    const GatherSeg& g = G.seg[s];
    const uint32_t* src = g.base + g.stride * (size_t)a + g.off;
    for (uint32_t w = lane; w < g.words; w += nlanes) row[g.at + w] = src[w];
  }
}

// pass 2, ego j: staging row j into its own segments
BMPC_HD void gather_commit_ego(const GatherList& G, const int32_t* anc, const uint32_t* stage, int j, int lane,
                               int nlanes) {
  if (gather_source(anc, G.batch, j) == j) return;
  const uint32_t* row = stage + (size_t)j * G.row_words;
  for (int s = 0; s < G.nseg; ++s) {
    const GatherSeg& g = G.seg[s];
    uint32_t* dst = g.base + g.stride * (size_t)j + g.off;
    for (uint32_t w = lane; w < g.words; w += nlanes) dst[w] = row[g.at + w];
  }
}

}  // namespace bmpc
