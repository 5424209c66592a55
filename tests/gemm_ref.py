"""Float64 references, per-element bars, operands and guarded outputs for the split-precision GEMMs of mma_amd/csrc/gemm_x3.hip
(tests/test_gemm_edges_gpu.py, tests/test_gemm_gpu.py), in the pattern of tests/tower_post_ref.py.

  NN   C (M,N) (+)= A (M,K) @ W (K,N)          nn64: ref, mag = |A| @ |W| (+ |C0| where accumulated)
  TN   C (KA,NC)  = X (M,KA)^T @ G (M,NC)      tn64: ref, mag = |X|^T @ |G|

Every bar is per ELEMENT: |got - ref| <= bar where mag, the sum of the magnitudes of the element's own terms, is positive, and got == 0
exactly where mag == 0.  No absolute floor and no global maximum: a column block that is wrong at 1e-3 of its own size does not pass because
another one is larger.

  C_X = 5e-7 of mag     the bar tests/test_gemm_gpu.py holds for every form, and the bar of every element here.  A wide range inside an
                        operand's row is fine for the six-product bf16 forms and the two-accumulator fp16 forms (every element keeps its
                        own 22+ bits).  The one exception is an element that a FEW TERMS DOMINATE: C_X is what a sum of many comparable
                        magnitudes shows, mag being far larger than any partial sum; where the terms of the rows spread over e^+-20
                        inside (or the lone 1e36) are more than half of mag, every addition of the fp32 accumulator rounds at their
                        scale and nothing averages.  Those elements - D > mag / 2, D the part of mag that the spread rows of the
                        population contribute, known from the population, not from the result - may exceed C_X, and are then held to
                        torch fp32 ON THE SAME ELEMENTS: max err / mag over them <= 1.5 * (torch fp32's) + 1e-7.  An element over C_X
                        anywhere else fails.  Met: bf16x3 5.74e-7 on a spread row (torch fp32 5.80e-7), the batched TN form 1.10e-6 on
                        elements of the spread rows (torch fp32 2.03e-6).
  + 2^-23 |c0|          accumulating calls: the one fp32 addition onto c0 (half an ulp of a sum that may be twice c0)
  tn_header_bound       mma_gemm_f16x2_tn, as include/mma_amd.h states it: 2^-22 sum|x||g| + M 2^-39 max_i(max|x_i| max|g_i|), with the
                        row maxima the CALLER passed (a loose bound scales the rows down, so the absolute term grows with it): the bar
                        of the cases that are about the bound (many comparable rows).
  three_product_bar     every other case of mma_gemm_f16x2_tn: C_X mag, + 3 * 2^-22 T on the elements whose largest single term T is more
                        than half of mag.  From the piece formats: hi = fp16(x) is off by up to 2^-11 |x| (half an ulp of 11 bits), lo =
                        fp16(x - hi) by up to 2^-11 of THAT, so one operand is kept to 2^-22 in the worst case, the other one too, and
                        the dropped lo lo term is up to 2^-22 |x||g|: ONE product can be off by 3 * 2^-22 = 7.2e-7 of itself.  2^-22 (the
                        header) and C_X are what a sum of many comparable terms shows; at M = 33 one row can be all of an element (met:
                        x = 32.017, its row maximum, times g = -0.008656 is 98 % of the element, off by 5.3e-7; the six-product kernel:
                        7.5e-9) - such an element has no crowd to average over, and T carries the worst case of its one term.
  nlp_header_bound      mma_gemm_f16x2_nlp: "22 bits for every element within 2^16 of its row / column maximum, an absolute 2^-25 of
                        the scaled maximum below".  The sentence gives no count for the absolute term; derived from the piece formats:
                          a row is scaled by s_i = 2^(14 - ea_i), ea_i = floor(log2 row_max_i), a column of W by t_j = 2^(14 - ew_j);
                          x = a s is kept as hi = fp16(x), lo = fp16(x - hi).  x - hi is exact in fp32; fp16(x - hi) keeps 11 bits of it
                          while it is a normal fp16 number (>= 2^-14) - the header's "22 bits", its relative term, taken as stated -
                          and is off by at most half the subnormal spacing, 2^-25, below.  So beside the relative term EVERY element
                          of either operand carries an absolute 2^-25 in scaled units.  Summed over k and un-scaled by 1 / (s_i t_j):
                            |err_ij| <= 2^-22 mag_ij                              (the header's 22 bits)
                                      + 2^-25 (2^(ea_i - 14) sum_k |w_kj| + 2^(ew_j - 14) sum_k |a_ik|)
                          i.e. K absolute terms per operand, each 2^-25 in scaled units: 2^-39 of the (power-of-two floor of the)
                          row / column maximum per term.  A loose row_max (8x) raises ea_i by 3.
  yardstick             the same product in torch fp32 on the GPU, e_f32 in the same units: over the pooled cases of a form with at
                        least 2^16 output elements, e_got <= 1.5 * e_f32 + 1e-7 (the form of tests/test_gemm_gpu.py).

Measured on an MI355X by tests/test_gemm_edges_gpu.py, in units of mag (e_got: the kernel, e_f32: torch fp32 on the same GPU, both against
float64; the largest of each over the pooled cases of the form with >= 2^16 output elements; `cases`: how many were pooled):
  form                  entry point                      e_got      e_f32      cases   where the pooled cases come from
  bf16x3                mma_gemm_bf16x3                  5.74e-07   5.80e-07   14      grid-stride, column groups 3 / 5 / 32, N = 128 long K, blocks
  f16x2_n128            mma_gemm_f16x2_n128              2.89e-07   3.41e-07   2       M = 65 536 + 257, K = 256, both accumulate values
  f16x2_nlp             mma_gemm_f16x2_nlp               2.58e-07   4.38e-07   4       M = 65 536 + 257, K = 256, N = 128 / 256, both accumulate values
  bf16x3_tn             mma_gemm_bf16x3_tn               4.40e-07   7.39e-07   1       (1000, 128, 640)
  f16x2_tn              mma_gemm_f16x2_tn                5.34e-07   3.61e-07   4       KA = 255 / 256, NC = 300, M = 33 / 1000 (eight waves)
  bf16x3_tn_batched     mma_gemm_bf16x3_tn_batched       8.53e-07   2.03e-06   8       (4129, 128, 640), B = 1, 2, 5, per tower
  The largest e_got of ANY case (the small ones included): bf16x3 5.74e-07 (a row spread over e^+-20 inside, N = 4096; torch fp32 on the
  same rows 5.80e-07) and 5.59e-07 (the same kind of row, M = 65 791, K = 256; torch fp32 4.05e-07), n128 4.56e-07 (its spread rows stay
  under C_X), nlp 2.59e-07 on ordinary rows (1.96e-04 of mag on the wide-row case, under the header's absolute term), k256 / k256p
  2.18e-07, f16x2_k 4.56e-07, bf16x3_tn 4.91e-07 (no element over C_X), f16x2_tn 5.34e-07 (M = 33, one row is the element:
  three_product_bar), batched 1.10e-06 ((8, 32), B = 5, tower 3: 63 elements that the spread rows dominate; torch fp32 on them 7.11e-07,
  and between 1.0e-06 and 2.0e-06 on the dominated elements of the other towers, where the kernel has 5.2e-07 .. 8.5e-07).
"""
import math
from collections import defaultdict

import numpy as np
import torch

DEV = "cuda:0"
C_X = 5e-7
EPS_ADD = 2.0 ** -23
# The guard cells of an fp32 output: one exactly representable finite value (1.3e36, every byte 0x7B) that no product of the operands
# below makes; compared as bits.
SENTINEL = 0x7B7B7B7B
GUARD_ABOVE, GUARD_BELOW, GUARD_LEFT, GUARD_RIGHT = 8, 32, 3, 5

# ---- thresholds that exist only inside gemm_x3.hip (mma_gemm_bf16x3, "tall plain K == 128 products ..." and "N == 128 with a long K"):
CG_ROWS = 256                    # kCgRows / kNlRows: rows of one unit of the 8-wave kernels


def colgroup_min_rows(N):
    """gemm_x3_colgroup_kernel is admitted from M / 256 >= 4 * 8 * (32 / n_groups) on (integer division, n_groups = N / 128)."""
    return CG_ROWS * 4 * 8 * (32 // (N // 128))


X3_N128_MIN_ROWS = 256 * 256     # gemm_x3_n128_kernel: N == 128, K > 128, M / 256 >= 256
GRID_X3 = 512                    # gemm_x3_kernel: at most 512 workgroups of 128 rows, then grid-stride
GRID_UNITS = 256                 # the 8-wave kernels: at most 256 workgroups of 256 rows, then grid-stride


# ---- references -----------------------------------------------------------------------------------------------------------------------
def nn64(a, w, c0=None):
    """(ref, mag) of c0 + a @ w in float64 on the device of a."""
    ref, mag = a.double() @ w.double(), a.double().abs() @ w.double().abs()
    if c0 is not None:
        ref, mag = ref + c0.double(), mag + c0.double().abs()
    return ref, mag


def tn64(x, g):
    """(ref, mag) of x^T @ g in float64."""
    return x.double().t() @ g.double(), x.double().abs().t() @ g.double().abs()


def nn32(a, w, c0=None):
    """The yardstick: the same product from torch's fp32 ops on the GPU."""
    p = a.contiguous() @ w
    return p if c0 is None else c0 + p


def floor_log2(v):
    """floor(log2 v) of positive float64 values, exactly (frexp), 0 where v == 0."""
    return torch.where(v > 0, torch.frexp(v.double())[1].double() - 1, torch.zeros_like(v, dtype=torch.float64))


def nlp_header_bound(a, w, row_max, mag):
    """The header's bound of mma_gemm_f16x2_nlp per element (derivation: module docstring); row_max: what the caller passed."""
    ea = floor_log2(row_max.double())                                  # (M,)
    ew = floor_log2(w.double().abs().amax(0))                          # (N,)
    ta = torch.where(row_max > 0, torch.exp2(ea - 14), torch.zeros_like(ea))
    tw = torch.exp2(ew - 14)
    return 2.0 ** -22 * mag + 2.0 ** -25 * (ta[:, None] * w.double().abs().sum(0)[None, :] + a.double().abs().sum(1)[:, None] * tw[None, :])


def largest_term(x, g):
    """(KA, NC) max_i |x_ik| |g_in|: the largest single term of every element of x^T g, 64 rows at a time."""
    xa, ga = x.double().abs(), g.double().abs()
    T = torch.zeros((x.shape[1], g.shape[1]), device=x.device, dtype=torch.float64)
    for r in range(0, x.shape[0], 64):
        T = torch.maximum(T, (xa[r:r + 64, :, None] * ga[r:r + 64, None, :]).amax(0))
    return T


def three_product_bar(x, g, mag, max_rows=4096):
    """C_X mag, + 3 * 2^-22 T where the largest term T is more than half of mag: module docstring.  Above max_rows C_X alone (the
    stricter bar)."""
    if x.shape[0] > max_rows:
        return C_X * mag
    T = largest_term(x, g)
    return C_X * mag + torch.where(T > 0.5 * mag, 3 * 2.0 ** -22 * T, torch.zeros_like(T))


def rows_of_kind(M, kinds, kind):
    """The rows edge_matrix(M, ..., kinds=kinds) gives `kind`."""
    rows = []
    for i, k in enumerate(kinds):
        if k == kind:
            if M - 1 - i >= 0:
                rows.append(M - 1 - i)
            if 3 + i < M - len(kinds):
                rows.append(3 + i)
    return rows


def tn_header_bound(x_row_max, g_row_max, mag, M):
    """|error| <= 2^-22 sum|x||g| + M 2^-39 max_i(max|x_i| max|g_i|) - the same absolute term for every element."""
    return 2.0 ** -22 * mag + M * 2.0 ** -39 * (x_row_max.double() * g_row_max.double()).max().item()


# ---- bars ------------------------------------------------------------------------------------------------------------------------------
def err_over(got, ref, unit):
    """max |got - ref| / unit over the elements with unit > 0; inf when an element with unit == 0 is not exactly 0 or anything is not
    finite."""
    assert got.shape == ref.shape == unit.shape, (got.shape, ref.shape, unit.shape)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    pos = unit > 0
    if bool((got[~pos] != 0).any()):
        return math.inf
    return ((got.double() - ref).abs()[pos] / unit[pos]).max().item() if bool(pos.any()) else 0.0


def assert_bar(what, got, ref, mag, c=C_X, bar=None, c0=None, dominated=None, f32=None):
    """Per element |got - ref| <= bar (default c * mag; accumulating calls: + 2^-23 |c0|), got == 0 where mag == 0, everything finite - a
    NaN pad column that leaked shows here.  Prints the figure before it asserts; returns e_got = max err / mag.
    dominated (the part of mag that the spread rows of the population contribute) and f32 (a function that returns torch fp32's result):
    elements over the bar are let through only if ALL of them have dominated > mag / 2, and then max err / mag over every such element
    must be <= 1.5 * (the same figure of torch fp32) + 1e-7 (module docstring)."""
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite elements (a pad column or a stale row leaked)" % (what, int((~torch.isfinite(got)).sum()))
    zero = mag == 0
    assert bool((got[zero] == 0).all()), "%s: %d elements with no term are not exactly 0" % (what, int((got[zero] != 0).sum()))
    if bar is None:
        bar = c * mag
    if c0 is not None:
        bar = bar + EPS_ADD * c0.double().abs()
    err = (got.double() - ref).abs()
    e_got = err_over(got, ref, mag)
    worst = (err - bar).max().item() if err.numel() else 0.0
    print("BAR %-60s e_got %.3e" % (what, e_got))
    if worst > 0 and dominated is not None:
        S = dominated > 0.5 * mag
        stray = (err > bar) & ~S
        if not bool(stray.any()):
            e_dom = (err[S] / mag[S]).max().item()
            e_f32 = ((f32().double() - ref).abs()[S] / mag[S]).max().item()
            print("DOM %-60s e_got %.3e  e_f32 %.3e on %d dominated elements" % (what, e_dom, e_f32, int(S.sum())))
            assert e_dom <= 1.5 * e_f32 + 1e-7, "%s: on the %d elements that the spread rows dominate e_got = %.4e, torch fp32 %.4e" % (
                what, int(S.sum()), e_dom, e_f32)
            return e_got
        err = torch.where(stray, err, torch.zeros_like(err))          # report an element that nothing dominates
        bar = torch.where(stray, bar, torch.full_like(err, math.inf))
    if worst > 0:
        i = int((err - bar).argmax())
        r, col = divmod(i, got.shape[1])
        raise AssertionError("%s: element (%d, %d) is off by %.4e, bar %.4e (%.3e of mag); e_got over the call %.3e"
                             % (what, r, col, err[r, col].item(), bar[r, col].item(), err[r, col].item() / max(mag[r, col].item(), 1e-300), e_got))
    return e_got


POOL = defaultdict(list)          # form -> [(e_got, e_f32, numel)]: the yardstick's pooled cases


def note_yardstick(form, got, f32, ref, mag):
    if got.numel() >= 1 << 16:
        POOL[form].append((err_over(got, ref, mag), err_over(f32, ref, mag), got.numel()))


def assert_yardstick(form):
    """Over the pooled cases of `form`: e_got <= 1.5 * e_f32 + 1e-7."""
    cases = POOL[form]
    assert cases, ("no case of %s with >= 2^16 output elements was pooled: the yardstick is taken over the cases that ran before it in this "
                   "process - run the whole file, in file order" % form)
    e_got, e_f32 = max(c[0] for c in cases), max(c[1] for c in cases)
    print("YARDSTICK %-24s e_got %.3e  e_f32 %.3e  cases %d" % (form, e_got, e_f32, len(cases)))
    assert e_got <= 1.5 * e_f32 + 1e-7, "%s: e_got = %.4e, e_f32 = %.4e over %d cases" % (form, e_got, e_f32, len(cases))
    return e_got, e_f32


# ---- operands --------------------------------------------------------------------------------------------------------------------------
def nan_padded(t, left, right):
    """t (rows, cols) as a row-strided view of a wider GPU buffer whose pad columns (left / right of it) are NaN."""
    rows, cols = t.shape
    buf = torch.full((rows, left + cols + right), float("nan"), device=DEV, dtype=torch.float32)
    buf[:, left:left + cols] = t.to(DEV)
    return buf[:, left:left + cols]


def pad_a(t):
    """A of the NN forms: a 16-byte aligned base and a pitch of whole float4s - 4 NaN floats on both sides."""
    v = nan_padded(t, 4, 4)
    assert v.data_ptr() % 16 == 0 and v.stride(0) % 4 == 0
    return v


def pad_x(t):
    """X / G of the TN forms: 4-byte alignment - one NaN float left, two right (an odd pitch)."""
    return nan_padded(t, 1, 2)


EDGE_KINDS = ("spread", "zero", "big", "tiny")


def edge_matrix(M, K, rng, relu=False, kinds=EDGE_KINDS, spread=20.0, big=1.0e36, tiny=1.0e-30, scale=1.0):
    """(M, K) float32 tensor (CPU): rows of standard normals scaled over e^+-6 against each other (relu: their negative part cut to zero),
    with a fixed population of edge rows counted from the END - row M-1 is the first of `kinds`, M-2 the second, ... - so that one edge row is
    the last row of the matrix and the others sit in the last (ragged) wavefront, and again from row 3 on where the matrix has room:
      spread  exp(U(-spread, spread)) inside the row        zero  all zero
      big     zero but for one `big` (1e36)                  tiny  zero but for one `tiny` (1e-30)
    scale multiplies the ordinary and the spread rows (an operand at 1e-3 whose lone values stay what they are)."""
    v = rng.standard_normal((M, K)) * np.exp(rng.uniform(-6, 6, (M, 1))) * scale
    if relu:
        v = np.maximum(v, 0)

    def put(r, kind):
        if kind == "spread":
            v[r] = rng.standard_normal(K) * np.exp(rng.uniform(-spread, spread, K)) * scale
        else:
            v[r] = 0.0
            if kind == "big":
                v[r, rng.integers(K)] = big
            elif kind == "tiny":
                v[r, rng.integers(K)] = tiny
    for i, kind in enumerate(kinds):
        if M - 1 - i >= 0:
            put(M - 1 - i, kind)
        if 3 + i < M - len(kinds):
            put(3 + i, kind)
    return torch.from_numpy(v.astype(np.float32))


def weights(K, N, rng, col_spread=3.0):
    """(K, N) uniform weights / sqrt(K), columns scaled over e^+-col_spread against each other (GPU)."""
    return torch.from_numpy(((rng.random((K, N)) * 2 - 1) / np.sqrt(K) * np.exp(rng.uniform(-col_spread, col_spread, (1, N)))).astype(np.float32)).to(DEV)


def mixed_row_max(a):
    """row_max as callers pass it: exact, 8x loose on every third row (row 0 among them), 0 on the all-zero rows."""
    rm = a.abs().amax(1).contiguous()
    rm[::3] *= 8.0
    return rm


# ---- guarded fp32 outputs ---------------------------------------------------------------------------------------------------------------
def guarded(M, N, fill=None):
    """(buffer, out): out (M, N) is a column block of a wider fp32 buffer - 3 guard columns left and 5 right, 8 guard rows above and 32
    below (a wavefront re-reads at most 31 rows past M, whose stores only a descriptor's range or a row select keeps out) - every guard
    cell = SENTINEL.  The guard rows are part of the allocation: a kernel that is wrong by up to 31 rows stays inside this buffer.
    fill: an (M, N) tensor or a number `out` starts from (default NaN: an element the kernel does not write shows as non-finite)."""
    buf = torch.full((M + GUARD_ABOVE + GUARD_BELOW, N + GUARD_LEFT + GUARD_RIGHT), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    out = buf[GUARD_ABOVE:GUARD_ABOVE + M, GUARD_LEFT:GUARD_LEFT + N]
    if torch.is_tensor(fill):
        out.copy_(fill)
    else:
        out.fill_(float("nan") if fill is None else fill)
    return buf, out


def assert_guards_intact(buf, M, N, what=""):
    b = buf.view(torch.int32).clone()
    b[GUARD_ABOVE:GUARD_ABOVE + M, GUARD_LEFT:GUARD_LEFT + N] = SENTINEL
    bad = b != SENTINEL
    if bool(bad.any()):
        r, c = [int(t[0]) for t in torch.nonzero(bad, as_tuple=True)]
        raise AssertionError("%s: %d guard cells overwritten, the first at row %d, column %d of out" % (what, int(bad.sum()), r - GUARD_ABOVE, c - GUARD_LEFT))


def guarded_flat(rows, cols, below=GUARD_BELOW):
    """(buffer, out) for a CONTIGUOUS (rows, cols) output (C of the TN forms, a workspace): guard rows above and below only."""
    buf = torch.full((rows + GUARD_ABOVE + below, max(cols, 1)), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    out = buf[GUARD_ABOVE:GUARD_ABOVE + rows]
    out.fill_(float("nan"))
    return buf, out


def guarded_vec(n):
    """(buffer, ws): n floats (a workspace), NaN, between 16 guard floats on either side (64 bytes: ws keeps the buffer's alignment)."""
    buf = torch.full((n + 32,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    buf[16:16 + n] = float("nan")
    return buf, buf[16:16 + n]


def assert_vec_guards_intact(buf, n, what=""):
    b = buf.view(torch.int32)
    bad = int((b[:16] != SENTINEL).sum()) + int((b[16 + n:] != SENTINEL).sum())
    assert bad == 0, "%s: %d guard cells overwritten" % (what, bad)


def assert_flat_guards_intact(buf, rows, what=""):
    b = buf.view(torch.int32)
    bad = int((b[:GUARD_ABOVE] != SENTINEL).sum()) + int((b[GUARD_ABOVE + rows:] != SENTINEL).sum())
    assert bad == 0, "%s: %d guard cells overwritten" % (what, bad)


# ---- dispatch, read from the project ----------------------------------------------------------------------------------------------------
REACHED = set()                   # every entry point any recorded call of the session reached


class Recorder:
    """Records the entry points reached through dense.call (the monkeypatch test_gemm_bf16_out_gpu.py uses for rows_to_bf16) and through
    .call / .query, the raw forms the tests use themselves."""

    def __init__(self, monkeypatch):
        from mma_amd import _lib, dense
        self.names, self._lib = [], _lib
        real = dense.call
        monkeypatch.setattr(dense, "call", lambda name, *a: (self._note(name), real(name, *a))[1])

    def _note(self, name):
        self.names.append(name)
        REACHED.add(name)

    def call(self, name, *args):
        self._note(name)
        return self._lib.call(name, *args)

    def query(self, name, *args):
        self._note(name)
        return self._lib.query(name, *args)

    def clear(self):
        del self.names[:]

    def assert_reached(self, *names):
        for n in names:
            assert n in self.names, "%s was not reached: %r" % (n, sorted(set(self.names)))

    def assert_only(self, *names):
        """Of the GEMM entry points, only `names` ran (the splits, row maxima and conversions beside them do not count)."""
        gemms = {n for n in self.names if n.startswith("mma_gemm_")}
        assert gemms == set(names), "GEMM entry points reached: %r, expected %r" % (sorted(gemms), sorted(names))


def tn_splits(M, KA, NC):
    """Row ranges mma_gemm_bf16x3_tn cuts M into - from the library's own workspace query (one (KA, NC) tile per split; 0 floats: one)."""
    from mma_amd import _lib
    return max(1, _lib.query("mma_gemm_bf16x3_tn_workspace_floats", M, KA, NC) // (KA * NC))


def tn_splits_batched(M, KA, NC, B):
    from mma_amd import _lib
    return max(1, _lib.query("mma_gemm_bf16x3_tn_batched_workspace_floats", M, KA, NC, B) // (B * KA * NC))


def tn_rows_per_split(M, splits):
    """tn_plan: whole 32-row chunks."""
    return -(-(-(-M // splits)) // 32) * 32


def hip_entry_points(path):
    """Names of the extern "C" functions a .hip file defines (the declaration of mma_col_sum inside gemm_x3.hip ends in ';': not one)."""
    import re
    src = open(path).read()
    return sorted(set(re.findall(r'^extern "C" (?:int|int64_t) (mma_\w+)\([^;{]*\{', src, flags=re.M)))
