// What the NC kernel files - nc_fused.hip (K1 / K2a / K2b) and nc_moments.hip (K1s / K2s) - share beside common.h: the row address of
// their kernels and the host side of their entry points (the plan's checks, the dropout parameters, the lane geometry, the grids and
// the run-time -> template dispatch).  What is specific to one file (the K-slices and the one-launch form of nc_fused.hip; the table
// check, the dropout form and the two item launches of nc_moments.hip) stays in that file.
#pragma once
#include <type_traits>
#include "common.h"

namespace mma {

// row * pitch as ONE v_mad_u64_u32: rows and pitches are < 2^31 (checked on the host), so the 64-bit product needs neither the
// sign extension nor the two extra quarter-rate v_mul_lo_u32 the int * int64 form compiles to (3 multiplies per gathered row)
__device__ __forceinline__ size_t row_off(int row, int64_t ld) { return (size_t)((uint64_t)(uint32_t)row * (uint64_t)(uint32_t)ld); }

// ------------------------------------------------------------------------------------------------------
// host side
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// a logit table's vector condition: one lane reads 4 elements at once - 16 bytes of fp32, 8 bytes of bf16
template <class TT> static bool table_aligned(const TT* p) { return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(TT) - 1)) == 0; }

// ---- the shared requirements of the entry points, in the order they have always made them: each file's nc_common_checks is
// nc_range_checks and its own H (/ K) line, and each entry point's own checks sit between the helpers.
static int nc_range_checks(int64_t N, int64_t E) {
  MMA_REQUIRE(N >= 0 && E >= 0 && N < (1LL << 31) && E < (1LL << 31), "N=%lld E=%lld out of int32 range", (long long)N, (long long)E);
  return 0;
}
// `partial` is fp32 (K1, K2b, K2s) or fp64 (K1s): only its presence is checked here
static int nc_item_checks(int64_t n_items, int64_t n_wave_items, const int32_t* hubs, int64_t n_hubs, const void* partial, int64_t n_slots) {
  MMA_REQUIRE(n_items >= 0 && n_hubs >= 0 && n_slots >= 0 && n_items < (1LL << 31) && n_wave_items >= 0, "negative or oversize item counts");
  MMA_REQUIRE(n_slots == 0 || (partial != nullptr && hubs != nullptr && n_hubs > 0), "hub slots without partial/hubs buffers");
  return 0;
}
static int nc_item_alignment(const int32_t* items, const int32_t* hubs) {
  MMA_REQUIRE(aligned16(items) && (hubs == nullptr || aligned16(hubs)), "items/hubs must be 16-byte aligned int32 quadruples");
  return 0;
}
// items [0, n_wave_items): one per wavefront; items [n_wave_items, n_items): one per LPR-lane group (short segments)
static int64_t nc_wave_items(int ipw, int64_t n_items, int64_t n_wave_items) {
  return (ipw == 1 || n_wave_items > n_items) ? n_items : n_wave_items;
}

// E >= 0 is checked before (nc_range_checks), so edge_base >= 0 && edge_base + E < 2^32 implies edge_base < 2^32: no clause of its own
static int make_drop(int32_t mode, uint32_t thr, uint64_t seed, const uint64_t* seed_dev, int64_t edge_base, const uint8_t* keep,
                     int64_t E, DropParams* d) {
  d->seed_dev = seed_dev;
  MMA_REQUIRE(edge_base >= 0 && edge_base + E < (1LL << 32), "drop_edge_base %lld out of range", (long long)edge_base);
  d->edge_base = (uint32_t)edge_base;
  MMA_REQUIRE(mode >= MMA_DROP_NONE && mode <= MMA_DROP_EXPLICIT, "drop_mode %d unknown", mode);
  MMA_REQUIRE(mode == MMA_DROP_NONE || thr < 65536, "drop_thr %u out of range (0..65535: P(drop) = thr / 65536)", thr);
  MMA_REQUIRE(mode != MMA_DROP_EXPLICIT || keep != nullptr, "drop_mode EXPLICIT needs a keep mask");
  drop_set_threshold(d, mode, thr);
  d->seed_lo = (uint32_t)seed; d->seed_hi = (uint32_t)(seed >> 32); d->keep = keep; d->E = E;
  return 0;
}

struct Geometry { int vec, lpr_log, chunks; };
// lanes per row: next power of two >= ceil(H/vec), at most one wave; wider rows take gridDim.y chunks
static Geometry geometry(int H, bool vec4_ok) {
  Geometry g;
  g.vec = vec4_ok ? 4 : 1;
  const int per_row = (H + g.vec - 1) / g.vec;
  g.lpr_log = min(ilog2_ceil(per_row), 6);
  g.chunks = (per_row + (1 << g.lpr_log) - 1) >> g.lpr_log;
  return g;
}

static dim3 item_grid(int64_t n_items, int chunks, int items_per_wave) {
  const int64_t per_block = (int64_t)(kBlock / kWave) * items_per_wave;
  int64_t blocks = (n_items + per_block - 1) / per_block;
  if (blocks > kMaxGrid) blocks = kMaxGrid;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks, (unsigned)chunks, 1);
}
static dim3 elementwise_grid(int64_t total) {
  int64_t b = (total + kBlock - 1) / kBlock;
  return dim3((unsigned)(b < 1 ? 1 : (b > kMaxGrid * 4 ? kMaxGrid * 4 : b)));
}

// run-time dropout mode -> template argument, beside ic / with_flag of common.h.
// EXPLICIT_OK = false: for kernels that are not instantiated for explicit masks (the one-launch kernels of nc_fused.hip).
template <bool EXPLICIT_OK = true, class F> static void with_dm(int dm, F&& f) {
  if (dm == MMA_DROP_HASH) f(ic<MMA_DROP_HASH>{});
  else if (dm == MMA_DROP_HASH16) f(ic<MMA_DROP_HASH16>{});
  else if (EXPLICIT_OK && dm == MMA_DROP_EXPLICIT) f(ic<EXPLICIT_OK ? MMA_DROP_EXPLICIT : MMA_DROP_NONE>{});
  else f(ic<MMA_DROP_NONE>{});
}

}  // namespace mma
