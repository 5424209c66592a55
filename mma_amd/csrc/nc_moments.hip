// K1s / K2s: the second-moment ("std") aggregator of the node-classification layer (include/mma_amd.h, ABI 37, bf16 tables: ABI 40;
// DESIGN.md "std aggregator"), hand-written for gfx950.  One mask, a kernel pair of its own on the NCGraph plan of K1 / K2b (nc_fused.hip):
//
//   forward   one pass over the by-target items: s1 = sum_j mu, s2 = sum_j mu^2 with mu = drop * a(P[i] + Q[j]) * x_j - and, when the
//             backward will run, T1 = sum_j drop x_j a' and T2 = sum_j mu drop x_j a' next to them, so that dL/dP is element-wise per node;
//   backward  one pass over the by-source items: per edge the target's P, g*r and mean rows are gathered, a / a' / the keep factor
//             recomputed, and e = g r (mu - mean) summed into gQ[j] = x_j sum e drop a' and gx[j] = sum e drop a.
//
// Lane mapping, item decode, index hand-out and the hub protocol are those of nc_fused.hip (a wavefront per long item, an LPR-lane
// group per short one, EPG neighbour rows per wave-instruction as 16-byte vectors when H % 4 == 0, two edge steps in flight; hub
// chunks leave partial sums that a finalize launch adds in slot order).  The variance is a difference of the FULL-segment sums: the
// sqrt / relu combine runs once per node, never per chunk.  No atomics anywhere: results are bitwise reproducible.
// The four forward sums are held in fp64 (the messages and their products are fp32 values; a 24 x 24-bit product is exact in fp64):
// msq - mean^2 and T2 - mean T1 cancel, and where the variance is small r = 1 / (d m) is up to 1 / (2 sqrt(1e-5)) = 158, which
// multiplies the rounding of fp32 sums into dL/dP (DESIGN.md "std aggregator").
// The accumulator set (four sums of one mask instead of one or two sums of K) and the gradient (it depends on the edge's own message,
// not on a per-target constant) are why this is not another instantiation of K1 / K2b.
// The logit tables P and Q are held as TT = float, or as bf16 in uint16_t (mma_nc_std_fwd_h / mma_nc_std_bwd_h): a compile-time
// parameter of the param structs and kernels, as in nc_fused.hip.  Exactly four loads see it (ldt / ldt_nt of common.h) - the forward's
// own P row and gathered Q rows, the backward's own Q row and gathered P rows; a value is widened with bits << 16, which is exact, so
// everything behind the load - the fp64 sums, x, g r, mean, every gradient - is the fp32 code, and the backward recomputes z from
// exactly what the forward read.
#include "nc_shared.h"

namespace mma {

constexpr float kStdEps = 1e-5f;      // layers.py:735

template <class TT>
struct NcStdFwdParams {
  const float* x; int64_t ldx;
  const TT* P; int64_t ldp; const TT* Q; int64_t ldq;       // pitches in elements
  const int32_t* rowptr; const int32_t* col;
  const int4* items; int64_t n_items;
  double* partial; int64_t pstride;  // fp64 values per slot: [s1 | s2] (2H), saving: [s1 | s2 | T1 | T2] (4H)
  float* m; int64_t ldm;
  float* saved; int64_t ldsv;        // (N, >= 3H): [mean | r | r (T2 - mean T1)]
  int H, lpr_log, raw;
  DropParams drop;
};

// keep factors of the VEC features at column c of edge e.  The std mask is mask 0 of a launch of its own: its HASH word is the base
// word itself, its EXPLICIT mask is (1,E,H).
template <int VEC, int DM>
__device__ __forceinline__ void std_keep(const DropParams& dp, uint32_t e, int c, int H, float (&f)[VEC]) {
  if (DM == MMA_DROP_HASH) {
    drop_unpack<VEC>(dp, drop_base_word(dp, e, c >> 2), c, f);
  } else if (DM == MMA_DROP_HASH16) {
    const uint32_t h = drop_base_word(dp, e, c >> 2);
    drop_unpack16<VEC>(dp, h, drop_low_word(h, drop_mask_mult2(0)), c, f);
  } else if (DM == MMA_DROP_EXPLICIT) {
    drop_explicit<VEC>(dp, e, 0, c, H, f);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) f[i] = 1.f;
  }
}

template <int VEC> struct DVec { double v[VEC]; };
template <int VEC> __device__ __forceinline__ DVec<VEC> dzero() {
  DVec<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = 0.0;
  return r;
}
// partial sums are few (hub chunks only): plain 8-byte accesses
template <int VEC> __device__ __forceinline__ DVec<VEC> std_dload(const double* p) {
  DVec<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = p[i];
  return r;
}
template <int VEC> __device__ __forceinline__ void std_dstore(double* p, const DVec<VEC>& a) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) p[i] = a.v[i];
}

// the combine of one (node, VEC columns) from its full-segment sums
template <int VEC, bool SAVE, class TT>
__device__ __forceinline__ void nc_std_write(const NcStdFwdParams<TT>& p, int node, int c, const DVec<VEC>& s1, const DVec<VEC>& s2,
                                             const DVec<VEC>& t1, const DVec<VEC>& t2) {
  const double d = (double)max(p.rowptr[node + 1] - p.rowptr[node], 1);
  Vec<VEC> mo, mean, r, coef;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    const double mn = s1.v[i] / d;
    const double var0 = s2.v[i] / d - mn * mn;
    const double vpos = var0 > 0.0 ? var0 : (var0 == var0 ? 0.0 : var0);     // relu that keeps a NaN, as torch's
    const double mv = sqrt(vpos + (double)kStdEps);
    mo.v[i] = (float)mv;
    if (SAVE) {
      const double rr = var0 > 0.0 ? 1.0 / (d * mv) : 0.0;                    // relu' is 0 at 0
      mean.v[i] = (float)mn;
      r.v[i] = (float)rr;
      coef.v[i] = (float)(rr * (t2.v[i] - mn * t1.v[i]));
    }
  }
  stv_nt<VEC>(p.m + row_off(node, p.ldm) + c, mo);
  if (SAVE) {
    float* sv = p.saved + row_off(node, p.ldsv) + c;
    stv<VEC>(sv, mean);                         // mean (and r, through g r) is re-read per edge by the backward: plain stores
    stv<VEC>(sv + p.H, r);
    stv_nt<VEC>(sv + 2 * (size_t)p.H, coef);
  }
}

// MULTI = false: one item per wavefront; MULTI = true: one item per group of G = LPR lanes (see nc_fwd_body in nc_fused.hip)
template <int VEC, bool SAVE, int DM, bool MULTI, class TT>
__global__ __launch_bounds__(kBlock, 2) void nc_std_fwd_kernel(const NcStdFwdParams<TT> p) {
  const DropParams dp = (DM == MMA_DROP_HASH || DM == MMA_DROP_HASH16) ? drop_resolve(p.drop) : p.drop;
  constexpr int U = 2;                          // edge steps in flight per lane
  const int lane = threadIdx.x & (kWave - 1);
  const int lpr = 1 << p.lpr_log;
  const int G = MULTI ? lpr : kWave;            // lanes per item
  const int epg = G >> p.lpr_log;               // neighbour rows a group gathers per step
  const int gpw = kWave / G;                    // items per wavefront
  const int grp = MULTI ? lane / G : 0;
  const int gl = lane & (G - 1);
  const int gbase = grp * G;
  const int sub = gl >> p.lpr_log;
  const int c = ((int)blockIdx.y * lpr + (lane & (lpr - 1))) * VEC;
  const bool fvalid = c < p.H;
  const int cc = fvalid ? c : 0;                // masked lanes read column 0 (valid memory), results are discarded
  const int waves_per_block = kBlock / kWave;
  const int64_t stride = (int64_t)gridDim.x * waves_per_block;
  const int64_t n_witems = (p.n_items + gpw - 1) / gpw;
  const bool raw = p.raw != 0;

  for (int64_t it0 = (int64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6); it0 < n_witems; it0 += stride) {
    int node, ebeg, eend, slot;
    bool ivalid = true;
    if (MULTI) {
      const int64_t idx = it0 * gpw + grp;
      ivalid = idx < p.n_items;
      const int4 item = p.items[ivalid ? idx : 0];
      node = item.x; ebeg = item.y; eend = ivalid ? item.z : item.y; slot = item.w;
    } else {
      const int4 item = p.items[__builtin_amdgcn_readfirstlane((int)it0)];
      node = __builtin_amdgcn_readfirstlane(item.x);
      ebeg = __builtin_amdgcn_readfirstlane(item.y);
      eend = __builtin_amdgcn_readfirstlane(item.z);
      slot = __builtin_amdgcn_readfirstlane(item.w);
    }
    const int len = eend - ebeg;
    int maxlen = len;
    if (MULTI) {
      for (int off = G; off < kWave; off <<= 1) maxlen = max(maxlen, __shfl_xor(maxlen, off, kWave));
      maxlen = __builtin_amdgcn_readfirstlane(maxlen);
    }

    const Vec<VEC> pi = ldt_nt<VEC>(p.P + row_off(node, p.ldp) + cc);
    DVec<VEC> s1 = dzero<VEC>(), s2 = dzero<VEC>(), t1 = dzero<VEC>(), t2 = dzero<VEC>();

    for (int base = 0; base < maxlen; base += G) {
      const int cnt = min(G, max(len - base, 0));      // edges of MY item in this index chunk
      const int ucnt = min(G, maxlen - base);          // wave-uniform trip bound
      const int myj = (gl < cnt) ? p.col[ebeg + base + gl] : 0;
      for (int t0 = 0; t0 < ucnt; t0 += U * epg) {
        int tt[U]; bool ev[U]; Vec<VEC> xj[U], qv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          tt[u] = t0 + u * epg + sub;
          ev[u] = tt[u] < cnt;
          const int j = __shfl(myj, gbase + (tt[u] & (G - 1)), kWave);
          const int jj = ev[u] ? j : node;     // inactive sub-rows re-read the item's own rows (cached); zeroed by the select below
          xj[u] = ldv<VEC>(p.x + row_off(jj, p.ldx) + cc);
          qv[u] = ldt<VEC>(p.Q + row_off(jj, p.ldq) + cc);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          // an inactive sub-row contributes exactly 0: its neighbour row is REPLACED by 0 (a product with 0 would turn an inf into NaN);
          // its logit comes from the item's own rows, so nothing foreign can leak in
#pragma unroll
          for (int i = 0; i < VEC; ++i) xj[u].v[i] = ev[u] ? xj[u].v[i] : 0.f;
          const uint32_t eu = (uint32_t)(ev[u] ? ebeg + base + tt[u] : 0);     // inactive: edge 0 (any valid position of the keep mask)
          float f[VEC];
          std_keep<VEC, DM>(dp, eu, cc, p.H, f);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float z = pi.v[i] + qv[u].v[i];
            float a, da;
            if (raw) { a = z; da = 1.f; }
            else { a = sigmoid_fast(z); da = a - a * a; }
            const float w = f[i] * xj[u].v[i];
            const double mu = (double)(a * w);           // the message is the fp32 value; its sums and products are exact-ish in fp64
            s1.v[i] += mu;
            s2.v[i] = fma(mu, mu, s2.v[i]);
            if (SAVE) {
              const double wd = (double)(da * w);
              t1.v[i] += wd;
              t2.v[i] = fma(mu, wd, t2.v[i]);
            }
          }
        }
      }
    }

    // butterfly over the sub-rows of a group (lanes with equal feature column)
    for (int off = G / 2; off >= lpr; off >>= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        s1.v[i] += __shfl_xor(s1.v[i], off, kWave);
        s2.v[i] += __shfl_xor(s2.v[i], off, kWave);
        if (SAVE) {
          t1.v[i] += __shfl_xor(t1.v[i], off, kWave);
          t2.v[i] += __shfl_xor(t2.v[i], off, kWave);
        }
      }
    }

    if (sub == 0 && fvalid && ivalid) {
      if (slot < 0) {
        nc_std_write<VEC, SAVE>(p, node, c, s1, s2, t1, t2);
      } else {
        double* ps = p.partial + (size_t)slot * p.pstride + c;
        std_dstore<VEC>(ps, s1);
        std_dstore<VEC>(ps + p.H, s2);
        if (SAVE) {
          std_dstore<VEC>(ps + 2 * (size_t)p.H, t1);
          std_dstore<VEC>(ps + 3 * (size_t)p.H, t2);
        }
      }
    }
  }
}

// hub nodes: the chunk partials summed in slot order (fixed: bitwise repeatable), then the same combine
template <int VEC, bool SAVE, class TT>
__global__ __launch_bounds__(kBlock) void nc_std_fwd_finalize_kernel(const NcStdFwdParams<TT> p, const int4* hubs, int64_t n_hubs) {
  const int per_row = (p.H + VEC - 1) / VEC;
  const int64_t total = n_hubs * per_row;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % per_row) * VEC;
    const int4 hub = hubs[idx / per_row];
    DVec<VEC> s1 = dzero<VEC>(), s2 = dzero<VEC>(), t1 = dzero<VEC>(), t2 = dzero<VEC>();
    for (int sl = hub.y; sl < hub.z; ++sl) {
      const double* ps = p.partial + (size_t)sl * p.pstride + c;
      const DVec<VEC> a = std_dload<VEC>(ps), b = std_dload<VEC>(ps + p.H);
      DVec<VEC> ct = dzero<VEC>(), dt = dzero<VEC>();
      if (SAVE) { ct = std_dload<VEC>(ps + 2 * (size_t)p.H); dt = std_dload<VEC>(ps + 3 * (size_t)p.H); }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        s1.v[i] += a.v[i]; s2.v[i] += b.v[i];
        if (SAVE) { t1.v[i] += ct.v[i]; t2.v[i] += dt.v[i]; }
      }
    }
    nc_std_write<VEC, SAVE>(p, hub.x, c, s1, s2, t1, t2);
  }
}

// ------------------------------------------------------------------------------------------------------
// backward, node level: gr = g * r (what the edge pass gathers per edge), gP = g * r (T2 - mean T1)
struct NcStdNodeParams {
  const float* g; int64_t ldg; const float* saved; int64_t ldsv;
  float* gr; int64_t ldgr; float* gP; int64_t ldgp;
  int64_t n_targets; int H;
};

template <int VEC>
__global__ __launch_bounds__(kBlock) void nc_std_bwd_node_kernel(const NcStdNodeParams p) {
  const int per_row = (p.H + VEC - 1) / VEC;
  const int64_t total = p.n_targets * per_row;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t node = idx / per_row;
    const int c = (int)(idx % per_row) * VEC;
    const Vec<VEC> g = ldv_nt<VEC>(p.g + (size_t)node * p.ldg + c);
    const float* sv = p.saved + (size_t)node * p.ldsv + c;
    const Vec<VEC> r = ldv_nt<VEC>(sv + p.H), coef = ldv_nt<VEC>(sv + 2 * (size_t)p.H);
    Vec<VEC> o1, o2;
#pragma unroll
    for (int i = 0; i < VEC; ++i) { o1.v[i] = g.v[i] * r.v[i]; o2.v[i] = g.v[i] * coef.v[i]; }
    stv<VEC>(p.gr + (size_t)node * p.ldgr + c, o1);         // gathered per edge next: plain store
    stv_nt<VEC>(p.gP + (size_t)node * p.ldgp + c, o2);
  }
}

// ------------------------------------------------------------------------------------------------------
// backward, edge level, over the transposed CSR (grouped by source j)
template <class TT>
struct NcStdBwdParams {
  const float* x; int64_t ldx;
  const TT* P; int64_t ldp; const TT* Q; int64_t ldq;
  const float* gr; int64_t ldgr; const float* mean; int64_t ldsv;      // mean = the first H columns of the saved rows
  const int32_t* t_col; const int32_t* t_eid;
  const int4* items; int64_t n_items;
  float* partial; int64_t pstride;   // floats per slot = 2H: [sum e drop a' | sum e drop a]
  float* gQ; int64_t ldgq; float* gx; int64_t ldgx;
  int H, lpr_log, raw;
  DropParams drop;
};

template <int VEC, int DM, bool MULTI, class TT>
__global__ __launch_bounds__(kBlock, 2) void nc_std_bwd_kernel(const NcStdBwdParams<TT> p) {
  constexpr bool DROP = DM != MMA_DROP_NONE;
  const DropParams dp = (DM == MMA_DROP_HASH || DM == MMA_DROP_HASH16) ? drop_resolve(p.drop) : p.drop;
  constexpr int U = 2;
  const int lane = threadIdx.x & (kWave - 1);
  const int lpr = 1 << p.lpr_log;
  const int G = MULTI ? lpr : kWave;
  const int epg = G >> p.lpr_log;
  const int gpw = kWave / G;
  const int grp = MULTI ? lane / G : 0;
  const int gl = lane & (G - 1);
  const int gbase = grp * G;
  const int sub = gl >> p.lpr_log;
  const int c = ((int)blockIdx.y * lpr + (lane & (lpr - 1))) * VEC;
  const bool fvalid = c < p.H;
  const int cc = fvalid ? c : 0;
  const int waves_per_block = kBlock / kWave;
  const int64_t stride = (int64_t)gridDim.x * waves_per_block;
  const int64_t n_witems = (p.n_items + gpw - 1) / gpw;
  const bool raw = p.raw != 0;

  for (int64_t it0 = (int64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6); it0 < n_witems; it0 += stride) {
    int node, ebeg, eend, slot;     // node = the SOURCE j
    bool ivalid = true;
    if (MULTI) {
      const int64_t idx = it0 * gpw + grp;
      ivalid = idx < p.n_items;
      const int4 item = p.items[ivalid ? idx : 0];
      node = item.x; ebeg = item.y; eend = ivalid ? item.z : item.y; slot = item.w;
    } else {
      const int4 item = p.items[__builtin_amdgcn_readfirstlane((int)it0)];
      node = __builtin_amdgcn_readfirstlane(item.x);
      ebeg = __builtin_amdgcn_readfirstlane(item.y);
      eend = __builtin_amdgcn_readfirstlane(item.z);
      slot = __builtin_amdgcn_readfirstlane(item.w);
    }
    const int len = eend - ebeg;
    int maxlen = len;
    if (MULTI) {
      for (int off = G; off < kWave; off <<= 1) maxlen = max(maxlen, __shfl_xor(maxlen, off, kWave));
      maxlen = __builtin_amdgcn_readfirstlane(maxlen);
    }

    const Vec<VEC> xj = ldv_nt<VEC>(p.x + row_off(node, p.ldx) + cc);
    const Vec<VEC> qj = ldt_nt<VEC>(p.Q + row_off(node, p.ldq) + cc);
    Vec<VEC> aq = vzero<VEC>(), ax = vzero<VEC>();

    for (int base = 0; base < maxlen; base += G) {
      const int cnt = min(G, max(len - base, 0));
      const int ucnt = min(G, maxlen - base);
      // lane 0 of a group with no edge in this chunk (but edges in an earlier one) offers the item's FIRST target: see the load phase
      const int myi = (gl < cnt) ? p.t_col[ebeg + base + gl] : ((gl == 0 && len > 0) ? p.t_col[ebeg] : 0);
      const int mye = (DROP && gl < cnt) ? p.t_eid[ebeg + base + gl] : 0;
      for (int t0 = 0; t0 < ucnt; t0 += U * epg) {
        bool ev[U]; uint32_t eid[U]; Vec<VEC> pv[U], gv[U], mv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int tt = t0 + u * epg + sub;
          ev[u] = tt < cnt;
          // A sub-row past the end of its item repeats the item's LAST valid edge of this index chunk (rows that are in flight or
          // cached anyway) and contributes exactly 0 through the select on e below - nothing FOREIGN is read.  A group with no edge
          // in this chunk repeats its item's first edge; an item with no edge at all reads target 0 and its sums are discarded.
          const int tl = min(tt, max(cnt - 1, 0));
          const int ii = __shfl(myi, gbase + (tl & (G - 1)), kWave);
          eid[u] = DROP ? (uint32_t)__shfl(mye, gbase + (tl & (G - 1)), kWave) : 0u;
          pv[u] = ldt<VEC>(p.P + row_off(ii, p.ldp) + cc);
          gv[u] = ldv<VEC>(p.gr + row_off(ii, p.ldgr) + cc);
          mv[u] = ldv<VEC>(p.mean + row_off(ii, p.ldsv) + cc);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          float f[VEC];
          std_keep<VEC, DM>(dp, eid[u], cc, p.H, f);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float z = pv[u].v[i] + qj.v[i];
            float a, da;
            if (raw) { a = z; da = 1.f; }
            else { a = sigmoid_fast(z); da = a - a * a; }
            const float mu = a * (f[i] * xj.v[i]);                       // the forward's message, same operation order
            const float e = ev[u] ? gv[u].v[i] * (mu - mv[u].v[i]) : 0.f;
            const float w = f[i] * e;
            aq.v[i] = fmaf(da, w, aq.v[i]);
            ax.v[i] = fmaf(a, w, ax.v[i]);
          }
        }
      }
    }

    for (int off = G / 2; off >= lpr; off >>= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        aq.v[i] += __shfl_xor(aq.v[i], off, kWave);
        ax.v[i] += __shfl_xor(ax.v[i], off, kWave);
      }
    }
    if (len == 0) {            // nothing was accumulated for this item (a chunk trip on behalf of other groups may have run)
      aq = vzero<VEC>();
      ax = vzero<VEC>();
    }

    if (sub == 0 && fvalid && ivalid) {
      if (slot < 0) {
        Vec<VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = xj.v[i] * aq.v[i];
        stv_nt<VEC>(p.gQ + row_off(node, p.ldgq) + c, o);
        stv_nt<VEC>(p.gx + row_off(node, p.ldgx) + c, ax);
      } else {
        float* ps = p.partial + (size_t)slot * p.pstride + c;
        stv<VEC>(ps, aq);
        stv<VEC>(ps + p.H, ax);
      }
    }
  }
}

template <int VEC, class TT>
__global__ __launch_bounds__(kBlock) void nc_std_bwd_finalize_kernel(const NcStdBwdParams<TT> p, const int4* hubs, int64_t n_hubs) {
  const int per_row = (p.H + VEC - 1) / VEC;
  const int64_t total = n_hubs * per_row;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % per_row) * VEC;
    const int4 hub = hubs[idx / per_row];
    Vec<VEC> aq = vzero<VEC>(), ax = vzero<VEC>();
    for (int sl = hub.y; sl < hub.z; ++sl) {                 // slot order: fixed
      const float* ps = p.partial + (size_t)sl * p.pstride + c;
      const Vec<VEC> a = ldv<VEC>(ps), b = ldv<VEC>(ps + p.H);
#pragma unroll
      for (int i = 0; i < VEC; ++i) { aq.v[i] += a.v[i]; ax.v[i] += b.v[i]; }
    }
    const int node = hub.x;
    const Vec<VEC> xj = ldv<VEC>(p.x + row_off(node, p.ldx) + c);
    Vec<VEC> o;
#pragma unroll
    for (int i = 0; i < VEC; ++i) o.v[i] = xj.v[i] * aq.v[i];
    stv_nt<VEC>(p.gQ + row_off(node, p.ldgq) + c, o);
    stv_nt<VEC>(p.gx + row_off(node, p.ldgx) + c, ax);
  }
}

// ------------------------------------------------------------------------------------------------------
// host side: what is specific to K1s / K2s; the checks, make_drop, geometry, the grids and with_dm are in nc_shared.h, with_flag in common.h
// a bf16 table at an odd address cannot be read at all (the scalar form loads 2-byte elements); fp32 tables are taken as they always were
template <class TT> static int std_table_checks(const TT* P, const TT* Q) {
  MMA_REQUIRE(sizeof(TT) != 2 || ((reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(Q)) & 1u) == 0,
              "bf16 tables P / Q at an odd address: they need 2-byte alignment");
  return 0;
}

static int nc_common_checks(int64_t N, int64_t E, int32_t H) {
  if (int rc = nc_range_checks(N, E)) return rc;
  MMA_REQUIRE(H >= 1 && H < (1 << 28), "H=%d unsupported", H);
  return 0;
}
// the kernels' dropout form: HASH with threshold 0 drops nothing, and so does any mode on a graph without edges
static int std_drop_form(int32_t mode, uint32_t thr, int64_t E, const DropParams& d) {
  return ((mode == MMA_DROP_HASH && thr == 0) || E == 0) ? MMA_DROP_NONE : d.mode;
}

// the two item launches: items [0, n_wave_items) one per wavefront, the rest one per LPR-lane group.  f(items, count, multi, grid)
template <class F>
static void std_for_parts(const int32_t* items, int64_t n_items, int64_t n_wave_items, const Geometry& g, F&& f) {
  const int ipw = kWave >> g.lpr_log;
  n_wave_items = nc_wave_items(ipw, n_items, n_wave_items);
  const int4* all = reinterpret_cast<const int4*>(items);
  if (n_wave_items > 0) f(all, n_wave_items, false, item_grid(n_wave_items, g.chunks, 1));
  if (n_items > n_wave_items) f(all + n_wave_items, n_items - n_wave_items, true, item_grid(n_items - n_wave_items, g.chunks, ipw));
}

}  // namespace mma

using namespace mma;

// mma_nc_std_fwd (TT = float) and mma_nc_std_fwd_h (TT = uint16_t: bf16 tables, pitches in elements)
template <class TT>
static int nc_std_fwd(
    const float* x, int64_t ldx, const TT* P, int64_t ldp, const TT* Q, int64_t ldq,
    const int32_t* rowptr, const int32_t* col,
    const int32_t* items, int64_t n_items, int64_t n_wave_items, const int32_t* hubs, int64_t n_hubs,
    double* partial, int64_t n_slots, float* m, int64_t ldms, float* saved, int64_t ldt,
    int64_t N, int64_t E, int32_t H, const uint8_t* act_host,
    int32_t drop_mode, uint32_t drop_thr, uint64_t seed, const uint64_t* seed_dev, int64_t drop_edge_base, const uint8_t* keep,
    void* stream) {
  if (int rc = nc_common_checks(N, E, H)) return rc;
  MMA_REQUIRE(act_host != nullptr, "NULL act_host");
  const int act = act_host[0];
  MMA_REQUIRE(act == MMA_ACT_SIGMOID || act == MMA_ACT_RAW, "act=%d is not an MMA_ACT_* code", act);
  MMA_REQUIRE(ldx >= H && ldp >= H && ldq >= H && ldms >= H, "row pitch too small: ldx=%lld ldp=%lld ldq=%lld ldms=%lld",
              (long long)ldx, (long long)ldp, (long long)ldq, (long long)ldms);
  MMA_REQUIRE(saved == nullptr || ldt >= 3LL * H, "ldt=%lld too small (3H)", (long long)ldt);
  MMA_REQUIRE(ldx < (1LL << 31) && ldp < (1LL << 31) && ldq < (1LL << 31) && ldms < (1LL << 31) && ldt < (1LL << 31), "row pitch out of range");
  if (int rc = nc_item_checks(n_items, n_wave_items, hubs, n_hubs, partial, n_slots)) return rc;
  if (N == 0 || n_items == 0) return 0;
  MMA_REQUIRE(x && P && Q && rowptr && items && m, "NULL argument");
  MMA_REQUIRE(E == 0 || col != nullptr, "NULL col");
  if (int rc = std_table_checks(P, Q)) return rc;
  if (int rc = nc_item_alignment(items, hubs)) return rc;
  MMA_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 7u) == 0, "partial must be 8-byte aligned (fp64 sums)");
  NcStdFwdParams<TT> p{};
  if (int rc = make_drop(drop_mode, drop_thr, seed, seed_dev, drop_edge_base, keep, E, &p.drop)) return rc;
  const int dm = std_drop_form(drop_mode, drop_thr, E, p.drop);
  const bool save = saved != nullptr;
  const bool v4 = (H % 4 == 0) && (ldx % 4 == 0) && (ldp % 4 == 0) && (ldq % 4 == 0) && (ldms % 4 == 0) && (!save || ldt % 4 == 0) &&
                  aligned16(x) && table_aligned(P) && table_aligned(Q) && aligned16(m) && (!save || aligned16(saved)) &&
                  (partial == nullptr || aligned16(partial));
  const Geometry g = geometry(H, v4);
  p.x = x; p.ldx = ldx; p.P = P; p.ldp = ldp; p.Q = Q; p.ldq = ldq; p.rowptr = rowptr; p.col = col;
  p.partial = partial; p.pstride = (save ? 4LL : 2LL) * H;
  p.m = m; p.ldm = ldms; p.saved = saved; p.ldsv = ldt;
  p.H = H; p.lpr_log = g.lpr_log; p.raw = act == MMA_ACT_RAW;
  hipStream_t st = static_cast<hipStream_t>(stream);
  std_for_parts(items, n_items, n_wave_items, g, [&](const int4* it, int64_t cnt, bool multi, dim3 grid) {
    p.items = it; p.n_items = cnt;
    with_flag(g.vec == 4, [&](auto v) { with_flag(save, [&](auto sv) { with_dm(dm, [&](auto d) { with_flag(multi, [&](auto mu) {
      hipLaunchKernelGGL((nc_std_fwd_kernel<decltype(v)::value ? 4 : 1, decltype(sv)::value, decltype(d)::value, decltype(mu)::value, TT>),
                         grid, dim3(kBlock), 0, st, p);
    }); }); }); });
  });
  if (int rc = check_launch("nc_std_fwd_kernel")) return rc;
  if (n_hubs > 0) {
    const int per_row = (H + g.vec - 1) / g.vec;
    const int4* hb = reinterpret_cast<const int4*>(hubs);
    with_flag(g.vec == 4, [&](auto v) { with_flag(save, [&](auto sv) {
      hipLaunchKernelGGL((nc_std_fwd_finalize_kernel<decltype(v)::value ? 4 : 1, decltype(sv)::value, TT>), elementwise_grid(n_hubs * per_row),
                         dim3(kBlock), 0, st, p, hb, n_hubs);
    }); });
    if (int rc = check_launch("nc_std_fwd_finalize_kernel")) return rc;
  }
  return 0;
}

// mma_nc_std_bwd (TT = float) and mma_nc_std_bwd_h (TT = uint16_t)
template <class TT>
static int nc_std_bwd(
    const float* x, int64_t ldx, const TT* P, int64_t ldp, const TT* Q, int64_t ldq,
    const float* g, int64_t ldg, const float* saved, int64_t ldt, float* gr, int64_t ldgr, float* gP, int64_t ldgp, int64_t n_targets,
    const int32_t* t_col, const int32_t* t_eid,
    const int32_t* items, int64_t n_items, int64_t n_wave_items, const int32_t* hubs, int64_t n_hubs,
    float* partial, int64_t n_slots, float* gQ, int64_t ldgq, float* gx, int64_t ldgx,
    int64_t N, int64_t E, int32_t H, const uint8_t* act_host,
    int32_t drop_mode, uint32_t drop_thr, uint64_t seed, const uint64_t* seed_dev, int64_t drop_edge_base, const uint8_t* keep,
    void* stream) {
  if (int rc = nc_common_checks(N, E, H)) return rc;
  MMA_REQUIRE(act_host != nullptr, "NULL act_host");
  const int act = act_host[0];
  MMA_REQUIRE(act == MMA_ACT_SIGMOID || act == MMA_ACT_RAW, "act=%d is not an MMA_ACT_* code", act);
  MMA_REQUIRE(ldx >= H && ldp >= H && ldq >= H && ldg >= H && ldt >= 3LL * H && ldgr >= H && ldgp >= H && ldgq >= H && ldgx >= H,
              "row pitch too small");
  MMA_REQUIRE(ldx < (1LL << 31) && ldp < (1LL << 31) && ldq < (1LL << 31) && ldg < (1LL << 31) && ldt < (1LL << 31) && ldgr < (1LL << 31) &&
              ldgp < (1LL << 31) && ldgq < (1LL << 31) && ldgx < (1LL << 31), "row pitch out of range");
  if (int rc = nc_item_checks(n_items, n_wave_items, hubs, n_hubs, partial, n_slots)) return rc;
  if (N == 0 || n_items == 0) return 0;
  MMA_REQUIRE(n_targets >= 1 && n_targets <= N, "n_targets=%lld: 1 <= n_targets <= N=%lld", (long long)n_targets, (long long)N);
  MMA_REQUIRE(x && P && Q && g && saved && gr && gP && items && gQ && gx, "NULL argument");
  MMA_REQUIRE(E == 0 || (t_col != nullptr && t_eid != nullptr), "NULL transposed CSR");
  if (int rc = std_table_checks(P, Q)) return rc;
  if (int rc = nc_item_alignment(items, hubs)) return rc;
  NcStdBwdParams<TT> p{};
  if (int rc = make_drop(drop_mode, drop_thr, seed, seed_dev, drop_edge_base, keep, E, &p.drop)) return rc;
  const int dm = std_drop_form(drop_mode, drop_thr, E, p.drop);
  const bool v4 = (H % 4 == 0) && (ldx % 4 == 0) && (ldp % 4 == 0) && (ldq % 4 == 0) && (ldg % 4 == 0) && (ldt % 4 == 0) && (ldgr % 4 == 0) &&
                  (ldgp % 4 == 0) && (ldgq % 4 == 0) && (ldgx % 4 == 0) && aligned16(x) && table_aligned(P) && table_aligned(Q) && aligned16(g) &&
                  aligned16(saved) && aligned16(gr) && aligned16(gP) && aligned16(gQ) && aligned16(gx) && (partial == nullptr || aligned16(partial));
  const Geometry geo = geometry(H, v4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int per_row = (H + geo.vec - 1) / geo.vec;
  {
    const NcStdNodeParams np{g, ldg, saved, ldt, gr, ldgr, gP, ldgp, n_targets, H};
    const dim3 grid = elementwise_grid(n_targets * per_row);
    if (geo.vec == 4) hipLaunchKernelGGL((nc_std_bwd_node_kernel<4>), grid, dim3(kBlock), 0, st, np);
    else hipLaunchKernelGGL((nc_std_bwd_node_kernel<1>), grid, dim3(kBlock), 0, st, np);
    if (int rc = check_launch("nc_std_bwd_node_kernel")) return rc;
  }
  p.x = x; p.ldx = ldx; p.P = P; p.ldp = ldp; p.Q = Q; p.ldq = ldq; p.gr = gr; p.ldgr = ldgr; p.mean = saved; p.ldsv = ldt;
  p.t_col = t_col; p.t_eid = t_eid; p.partial = partial; p.pstride = 2LL * H;
  p.gQ = gQ; p.ldgq = ldgq; p.gx = gx; p.ldgx = ldgx;
  p.H = H; p.lpr_log = geo.lpr_log; p.raw = act == MMA_ACT_RAW;
  std_for_parts(items, n_items, n_wave_items, geo, [&](const int4* it, int64_t cnt, bool multi, dim3 grid) {
    p.items = it; p.n_items = cnt;
    with_flag(geo.vec == 4, [&](auto v) { with_dm(dm, [&](auto d) { with_flag(multi, [&](auto mu) {
      hipLaunchKernelGGL((nc_std_bwd_kernel<decltype(v)::value ? 4 : 1, decltype(d)::value, decltype(mu)::value, TT>), grid, dim3(kBlock), 0, st, p);
    }); }); });
  });
  if (int rc = check_launch("nc_std_bwd_kernel")) return rc;
  if (n_hubs > 0) {
    const int4* hb = reinterpret_cast<const int4*>(hubs);
    const dim3 fg = elementwise_grid(n_hubs * per_row);
    if (geo.vec == 4) hipLaunchKernelGGL((nc_std_bwd_finalize_kernel<4, TT>), fg, dim3(kBlock), 0, st, p, hb, n_hubs);
    else hipLaunchKernelGGL((nc_std_bwd_finalize_kernel<1, TT>), fg, dim3(kBlock), 0, st, p, hb, n_hubs);
    if (int rc = check_launch("nc_std_bwd_finalize_kernel")) return rc;
  }
  return 0;
}

#define NC_STD_FWD_ARGS x, ldx, P, ldp, Q, ldq, rowptr, col, items, n_items, n_wave_items, hubs, n_hubs, partial, n_slots, m, ldms, saved, ldt, \
                        N, E, H, act_host, drop_mode, drop_thr, seed, seed_dev, drop_edge_base, keep, stream
extern "C" int mma_nc_std_fwd(
    const float* x, int64_t ldx, const float* P, int64_t ldp, const float* Q, int64_t ldq,
    const int32_t* rowptr, const int32_t* col,
    const int32_t* items, int64_t n_items, int64_t n_wave_items, const int32_t* hubs, int64_t n_hubs,
    double* partial, int64_t n_slots, float* m, int64_t ldms, float* saved, int64_t ldt,
    int64_t N, int64_t E, int32_t H, const uint8_t* act_host,
    int32_t drop_mode, uint32_t drop_thr, uint64_t seed, const uint64_t* seed_dev, int64_t drop_edge_base, const uint8_t* keep,
    void* stream) {
  return nc_std_fwd<float>(NC_STD_FWD_ARGS);
}
extern "C" int mma_nc_std_fwd_h(
    const float* x, int64_t ldx, const uint16_t* P, int64_t ldp, const uint16_t* Q, int64_t ldq,
    const int32_t* rowptr, const int32_t* col,
    const int32_t* items, int64_t n_items, int64_t n_wave_items, const int32_t* hubs, int64_t n_hubs,
    double* partial, int64_t n_slots, float* m, int64_t ldms, float* saved, int64_t ldt,
    int64_t N, int64_t E, int32_t H, const uint8_t* act_host,
    int32_t drop_mode, uint32_t drop_thr, uint64_t seed, const uint64_t* seed_dev, int64_t drop_edge_base, const uint8_t* keep,
    void* stream) {
  return nc_std_fwd<uint16_t>(NC_STD_FWD_ARGS);
}
#undef NC_STD_FWD_ARGS

#define NC_STD_BWD_ARGS x, ldx, P, ldp, Q, ldq, g, ldg, saved, ldt, gr, ldgr, gP, ldgp, n_targets, t_col, t_eid, items, n_items, n_wave_items, \
                        hubs, n_hubs, partial, n_slots, gQ, ldgq, gx, ldgx, N, E, H, act_host, drop_mode, drop_thr, seed, seed_dev, \
                        drop_edge_base, keep, stream
extern "C" int mma_nc_std_bwd(
    const float* x, int64_t ldx, const float* P, int64_t ldp, const float* Q, int64_t ldq,
    const float* g, int64_t ldg, const float* saved, int64_t ldt, float* gr, int64_t ldgr, float* gP, int64_t ldgp, int64_t n_targets,
    const int32_t* t_col, const int32_t* t_eid,
    const int32_t* items, int64_t n_items, int64_t n_wave_items, const int32_t* hubs, int64_t n_hubs,
    float* partial, int64_t n_slots, float* gQ, int64_t ldgq, float* gx, int64_t ldgx,
    int64_t N, int64_t E, int32_t H, const uint8_t* act_host,
    int32_t drop_mode, uint32_t drop_thr, uint64_t seed, const uint64_t* seed_dev, int64_t drop_edge_base, const uint8_t* keep,
    void* stream) {
  return nc_std_bwd<float>(NC_STD_BWD_ARGS);
}
extern "C" int mma_nc_std_bwd_h(
    const float* x, int64_t ldx, const uint16_t* P, int64_t ldp, const uint16_t* Q, int64_t ldq,
    const float* g, int64_t ldg, const float* saved, int64_t ldt, float* gr, int64_t ldgr, float* gP, int64_t ldgp, int64_t n_targets,
    const int32_t* t_col, const int32_t* t_eid,
    const int32_t* items, int64_t n_items, int64_t n_wave_items, const int32_t* hubs, int64_t n_hubs,
    float* partial, int64_t n_slots, float* gQ, int64_t ldgq, float* gx, int64_t ldgx,
    int64_t N, int64_t E, int32_t H, const uint8_t* act_host,
    int32_t drop_mode, uint32_t drop_thr, uint64_t seed, const uint64_t* seed_dev, int64_t drop_edge_base, const uint8_t* keep,
    void* stream) {
  return nc_std_bwd<uint16_t>(NC_STD_BWD_ARGS);
}
#undef NC_STD_BWD_ARGS
