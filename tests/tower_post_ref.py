"""Float64 restatements of the post-NN kernels (mma_amd/csrc/tower_post.hip: K13, K14, K15 and K16, the plain skinny Linear on the same
kernels), written from their formulas, the per-element bars their tests use (tests/test_tower_post_edges_gpu.py,
tests/test_tower_post_gpu.py) and the row population that makes a split or a select show.

  K13  y[n,t,o]        = sum_q pre_q(deg_n) sum_kf agg[n,t,kf] Wo[t][o][q*KF + kf]        pre_q = prod_{q' <= q} scaler_q'(clamp(deg_n, 1))
  K14  gagg[n,t,kf]    = sum_{q,o} pre_q gy[n,t,o] Wo[t][o][q*KF + kf]
  K15  gWo[t][o][q*KF+kf] = sum_n pre_q gy[n,t,o] agg[n,t,kf]
  K16  y = x W^T + b,  gx = gy W,  gW = gy^T x,  gb = column sums of gy

Every bar is per ELEMENT: |got - ref| <= c * mag where mag, the sum of the magnitudes of the element's own terms, is positive, and
got == 0 exactly where mag == 0.  There is no absolute floor - a floor hides the small rows - and no global maximum: a tower or a
column that is wrong at 1e-3 of its own size does not pass because another one is larger.

  C_Y  = 3e-7   K13 / K16 forward: the bar both forms (three bf16 pieces, exact fp32) already hold (test_tower_post_gpu.py)
  C_GW = 1e-6   K15 and its plain form: the bar of test_skinny_weight_and_bias_gradient_in_one_pass
  c_ga          K14 and K16's dL/dx: not a constant.  The same expression in torch fp32 on the GPU is measured against float64 in the
                same units (e_f32 = max err / mag); the kernel stays under 1.5 * e_f32 + 1e-7 (the form of test_gemm_gpu.py) AND under the
                derived worst case (S*16 + 2) * 2^-24: one rounding of pre * gy, then an fp32 chain over S*16 terms.
  pre           mma_tower_post_pre against pre64, relative per element: 2 * (torch fp32's own error) + 2^-23.

Measured on an MI355X, in units of mag (e_got: the kernel, e_f32: torch fp32 on the same GPU, both against float64; the largest e_got
of each group of cases in tests/test_tower_post_edges_gpu.py with the e_f32 of that case):
  K14 gagg (N, T, KF, O, S)                      e_got      e_f32      (S*16 + 2) * 2^-24
    (1, 1, 4, 1, 1)                              5.17e-08   5.17e-08   1.07e-06
    (321, 3, 36, 15, 3)   1, 2, 3, 8 tiles       2.18e-07   2.30e-07   2.98e-06
    (1153, 2, 100, 7, 2)  1, 2, 3, 8 tiles       2.89e-07   2.97e-07   2.03e-06
    (78400, 5, 4, 3, 1)   the planner's 3 tiles  1.53e-07   1.53e-07   1.07e-06
    (N, 2, 36, 15, 3)     N = 1 .. 130           2.76e-07   2.03e-07   2.98e-06      (N = 130; N = 1: 7.63e-08 / 6.48e-08)
    (130, 2, 416, 16, 4)                         2.73e-07   2.36e-07   3.93e-06
    (130, 2, 420, 16, 4)                         2.64e-07   2.54e-07   3.93e-06
    (130, 1, 480, 16, 4)                         2.14e-07   2.53e-07   3.93e-06
    (130, 1, 384, 7, 5)                          2.14e-07   2.72e-07   4.89e-06
    (130, 1, 512, 16, 3)                         2.43e-07   3.11e-07   2.98e-06
    (1000, 5, 152, 15, 3) edge rows              3.52e-07   3.32e-07   2.98e-06
    (4097, 3, 36, 16, 5)  edge rows              3.02e-07   3.01e-07   4.89e-06
    raw entry, (65 | 321, 3, 36 | 37, 15, 3)     2.71e-07   2.68e-07   2.98e-06
  K16 gx (N, K, O)
    (4161, 75, 75)        1, 2, 3, 8 tiles       2.69e-07   2.89e-07   4.89e-06
    (4200, 128, 16)                              2.46e-07   2.37e-07   1.07e-06
    (4161, 50, 80)                               3.11e-07   3.11e-07   4.89e-06
    (131136, 8, 5)        the planner's 2 tiles  1.97e-07   1.97e-07   1.07e-06
    (4160, 512, 48)                              3.05e-07   3.14e-07   2.98e-06
    (4160, 384, 80)                              3.81e-07   3.29e-07   4.89e-06
    (4160, 416, 64)                              3.50e-07   3.54e-07   3.93e-06
    (4160, 320, 80)                              2.93e-07   3.00e-07   4.89e-06
    (5000, 75, 75)        edge rows              2.50e-07   2.58e-07   4.89e-06
    raw entry, (65 | 321, 36 | 37, 45)           2.32e-07   1.96e-07   2.98e-06
  mma_tower_post_pre, relative (degrees 0, 1, 2, 10^6, 3 .. 299)
    all five scalers                             1.81e-07   2.38e-07
    all five, reversed                           1.91e-07   3.07e-07
    amplification, attenuation, linear           1.81e-07   1.76e-07
  Forward (C_Y): the largest e_got is 2.81e-07, the exact-fp32 kernel at (4161, 75, 75) under MMA_SKINNY_X3=0; the bf16-piece kernels stay
  under 1.9e-07.  K16 at (4160, 384, 80) - no bf16-piece form, one fp32 chain over 384 products - sat at 3.116e-07 (torch fp32: 3.22e-07)
  until the fp32 forward of such shapes summed round by round (tower_post_fwd_kernel<.., BLOCKED>): 6.99e-08.
  K15 (C_GW): the largest e_got is 6.39e-07, (1000, 5, 152, 15, 3) on edge rows.
  Subnormal pieces: no tiny row (e^-6 row scale, a lone 1e-30, e^-14 inside a row) came near a bar - nothing to write down.
"""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -24
C_Y = 3e-7
C_GW = 1e-6
SC = ["identity", "amplification", "attenuation", "linear", "inverse_linear"]



def pre64(deg, scalers, avg_log, avg_lin, dtype=torch.float64):
    """(N, S) running products of the degree scalers, in the reference's multiplication order ((1 f0) f1) ... (mma_conv.py:181-196).
    float64 is the truth; dtype=torch.float32 on a GPU tensor is the yardstick (what torch's fp32 ops make of the same formula)."""
    d = deg.clamp(min=1).to(dtype)
    lg = torch.log(d + 1)
    f = {"identity": torch.ones_like(d), "amplification": lg / avg_log, "attenuation": avg_log / lg, "linear": d / avg_lin, "inverse_linear": avg_lin / d}
    run, out = torch.ones_like(d), []
    for s in scalers:
        run = run * f[s]
        out.append(run)
    return torch.stack(out, 1)


def tower_post64(agg, Wo, pre, cot):
    """agg (N,T,KF), Wo (T,O,S*KF), pre (N,S), cot (N,T*O) -> dict of float64 tensors: y (N,T*O), gagg (N,T,KF), gWo (T,O,S*KF) and the
    per-element magnitudes mag_y, mag_ga, mag_gw (the same sums over the absolute values of the factors)."""
    N, T, KF = agg.shape
    O, S = Wo.shape[1], pre.shape[1]
    a, w, p = agg.double(), Wo.double().view(T, O, S, KF), pre.double()
    g = cot.double().view(N, T, O)

    def three(a, w, p, g):
        gs = g.unsqueeze(-1) * p.view(N, 1, 1, S)                      # (N,T,O,S): pre_q gy, the left operand of K14 and K15
        y = (torch.einsum("ntk,toqk->ntoq", a, w) * p.view(N, 1, 1, S)).sum(-1).reshape(N, T * O)
        return y, torch.einsum("ntoq,toqk->ntk", gs, w), torch.einsum("ntoq,ntk->toqk", gs, a).reshape(T, O, S * KF)

    y, ga, gw = three(a, w, p, g)
    my, mga, mgw = three(a.abs(), w.abs(), p.abs(), g.abs())
    return dict(y=y, gagg=ga, gWo=gw, mag_y=my, mag_ga=mga, mag_gw=mgw)


def tower_post32(agg, Wo, pre, cot):
    """The yardstick of c_ga: gagg from plain torch fp32 ops on the device of its arguments (pre: the fp32 table of that device)."""
    N, T, KF = agg.shape
    O, S = Wo.shape[1], pre.shape[1]
    gs = cot.view(N, T, O, 1) * pre.view(N, 1, 1, S)
    return torch.einsum("ntoq,toqk->ntk", gs, Wo.view(T, O, S, KF))


def linear64(x, W, b, cot):
    """x (N,K), W (O,K), b (O) or None, cot (N,O) -> dict: y, gx, gW, gb and mag_y, mag_gx, mag_gw, mag_gb in float64."""
    x, W, g = x.double(), W.double(), cot.double()
    b = b.double() if b is not None else None
    return dict(y=x @ W.t() + (b if b is not None else 0), gx=g @ W, gW=g.t() @ x, gb=g.sum(0),
                mag_y=x.abs() @ W.abs().t() + (b.abs() if b is not None else 0), mag_gx=g.abs() @ W.abs(), mag_gw=g.abs().t() @ x.abs(),
                mag_gb=g.abs().sum(0))


def err_over_mag(got, ref, mag):
    """max |got - ref| / mag over the elements with mag > 0; inf when an element with mag == 0 is not exactly 0 or anything is not
    finite.  The unit every bar here is stated in."""
    got, ref, mag = got.detach().cpu().double(), ref.detach().cpu().double(), mag.detach().cpu().double()
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    if not torch.isfinite(got).all():
        return math.inf
    pos = mag > 0
    if (got[~pos] != 0).any():
        return math.inf
    return ((got - ref).abs()[pos] / mag[pos]).max().item() if pos.any() else 0.0


def assert_bar(what, got, ref, mag, c):
    e = err_over_mag(got, ref, mag)
    print("BAR %-44s e_got %.3e  bar %.3e" % (what, e, c))
    assert e <= c, "%s: max |got - ref| / mag = %.4e, bar %.4e" % (what, e, c)
    return e


def ga_bar(S):
    """The derived worst case of K14 / K16's dL/dx: one rounding of pre * gy and an fp32 chain over S*16 terms."""
    return (S * 16 + 2) * EPS32


def assert_ga_bar(what, got, torch32, ref, mag, S):
    """c_ga: under 1.5 * e_f32 + 1e-7 and under (S*16 + 2) * 2^-24; prints both figures before it asserts."""
    e_got, e_f32 = err_over_mag(got, ref, mag), err_over_mag(torch32, ref, mag)
    print("GA  %-44s e_got %.3e  e_f32 %.3e  derived %.3e" % (what, e_got, e_f32, ga_bar(S)))
    assert e_got <= 1.5 * e_f32 + 1e-7, "%s: e_got = %.4e, e_f32 = %.4e" % (what, e_got, e_f32)
    assert e_got <= ga_bar(S), "%s: e_got = %.4e above the derived worst case %.4e" % (what, e_got, ga_bar(S))
    return e_got, e_f32


def edge_rows(a, rng, first=3):
    """The row population of the GEMM tests (test_gemm_f16x2_edge_rows), applied to the (rows, ...) fp32 tensor a; returns a new tensor.
    Row sizes spread by exp(U(-6, 6)); row `first` all zero; `first + 1` zero but for one 1e30; `first + 2` zero but for one 1e-30;
    `first + 3` with exp(U(-14, 0)) inside it; the last row zero.  Values stay inside [1e-30, 1e30] in magnitude (or are 0).
    `first` lets two operands of one product keep their 1e30 rows apart (1e30 * 1e30 is not an fp32 number)."""
    v = a.detach().cpu().numpy().astype(np.float64)
    rows = v.shape[0]
    flat = v.reshape(rows, -1)
    flat *= np.exp(rng.uniform(-6, 6, (rows, 1)))
    if rows > first + 3:
        flat[first] = 0.0
        flat[first + 1] = 0.0
        flat[first + 1, rng.integers(flat.shape[1])] = 1.0e30
        flat[first + 2] = 0.0
        flat[first + 2, rng.integers(flat.shape[1])] = 1.0e-30
        flat[first + 3] = rng.standard_normal(flat.shape[1]) * np.exp(rng.uniform(-14, 0, flat.shape[1]))
    flat[rows - 1] = 0.0
    nz = flat != 0
    flat[nz] = np.sign(flat[nz]) * np.clip(np.abs(flat[nz]), 1.0e-30, 1.0e30)
    return torch.from_numpy(flat.reshape(v.shape).astype(np.float32))


def edge_degrees(N, rng, hub_row=20):
    """Degrees 0 .. 6 with a 0 (clamped to 1), a 1 and one hub of 10^6 - the hub away from the 1e30 rows of edge_rows."""
    deg = torch.from_numpy(rng.integers(0, 7, N))
    deg[0] = 0
    if N > 1:
        deg[1] = 1
    if N > hub_row:
        deg[hub_row] = 10 ** 6
    return deg


def rowptr_of(deg):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg, 0)]).to(torch.int32)


def tiles_per_wave(N, T):
    """What post_tiles_per_wave() (tower_post.hip) plans with no sweep variable set - restated so that a test of a 'natural' plan can say
    that its shape still reaches the multi-tile path."""
    blocks1 = -(-(-(-N // 64)) // 4) * T
    best, best_cost = 1, -(-blocks1 // 512)
    for r in range(2, 9):
        blocks = -(-blocks1 // r)
        if blocks < (256 if T == 1 else 512):
            break
        cost = -(-blocks // 512) * r
        if cost <= best_cost:
            best, best_cost = r, cost
    return best
