"""GPU tests of the `std` aggregator of mma_amd.MMA (strict_reference=False; kernels: csrc/nc_moments.hip) against a plain torch
restatement of its definition (mma_amd/layers.py docstring, DESIGN.md "std aggregator"): float64 on the CPU is the truth, the same
statement in float32 on the CPU the reference value, and the bar is the project's own (golden_util.check_close with truth:
1e-5 + 1e-5|ref| + 6 x the row noise of the fp32 reference).  Compared: m, dL/dx and dL/dmask_std.

Shapes are the smallest at which the kernels take another path: the graphs of tests/nc_layer_util.py (degrees around the group /
wavefront item split and the 64-index chunk, a hub cut into partial slots, forward and transposed), H = 8 / 20 / 128 and one H that
is no multiple of 4.  This file's own defaults: fp32 tables, the weights as drawn, x uniform in [-1, 1]."""
import functools
import math

import numpy as np
import pytest
import torch

from golden_util import check_close
from nc_layer_util import (BOUNDARY as _BOUNDARY, C_OUT, DEV, HUB as _HUB, degenerate_targets, normalized_adj, oracle_with_grads, run_std,
                           small_graph, std_inputs as inputs, std_oracle)
import nc_layer_util

pytestmark = pytest.mark.gpu
SQRT_EPS = math.sqrt(1e-5)
make_layer = functools.partial(nc_layer_util.make_layer, strict_reference=False)


def compare(got, x, W, add_all, activation, cot, what, keep=None, p=0.0):
    truth = oracle_with_grads(x, W, add_all, activation, cot, keep, p, torch.float64)
    want = oracle_with_grads(x, W, add_all, activation, cot, keep, p, torch.float32)
    for g, w, t, name in zip(got, want, truth, ("m", "gx", "gmask_std")):
        err = np.abs(g.detach().cpu().numpy().astype(np.float64) - t)
        print("%s/%s: max |got - fp64| %.3g, max |fp32 ref - fp64| %.3g" % (what, name, err.max(), np.abs(w.astype(np.float64) - t).max()))
        check_close(g, w, None, None, what=what + "/" + name, signed_sum=True, truth=t)


# ---- 1 + 3: item boundaries x widths x activations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["sigmoid", "new_sigmoid"])
@pytest.mark.parametrize("H", [8, 20, 128, 6])
def test_item_boundaries(H, activation):
    layer = make_layer(_BOUNDARY, H, ["std"], activation, chunk=512)        # chunk > 65: every segment is one item
    g = layer.graph(torch.device(DEV))
    assert g.n_slots == 0 and g.t_n_slots == 0
    x, cot = inputs(_BOUNDARY, H)
    got = run_std(layer, x, cot)
    compare(got, x, layer.mask_std.detach().cpu(), _BOUNDARY, activation, cot, "std/boundary/H%d/%s" % (H, activation))


# ---- 2: a hub in partial slots, forward and transposed -------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [128, 6])
def test_hub_chunks(H):
    x, cot = inputs(_HUB, H)
    small = make_layer(_HUB, H, ["std"], chunk=32)
    whole = make_layer(_HUB, H, ["std"], chunk=512)
    with torch.no_grad():
        whole.mask_std.copy_(small.mask_std)
    g = small.graph(torch.device(DEV))
    hubs, t_hubs = g.hubs.cpu().numpy(), g.t_hubs.cpu().numpy()
    assert g.n_slots == 7 and hubs[:, 0].tolist() == [0] and g.t_n_slots == 7 and t_hubs[:, 0].tolist() == [1]       # ceil(200 / 32) slots
    assert whole.graph(torch.device(DEV)).n_slots == 0
    a, b, w = run_std(small, x, cot), run_std(small, x, cot), run_std(whole, x, cot)
    for u, v in zip(a, b):
        assert torch.equal(u, v)                                # fixed slot order, no atomics: bit-equal runs
    W = small.mask_std.detach().cpu()
    compare(a, x, W, _HUB, "sigmoid", cot, "std/hub/H%d/chunk32" % H)
    compare(w, x, W, _HUB, "sigmoid", cot, "std/hub/H%d/whole" % H)
    truth = oracle_with_grads(x, W, _HUB, "sigmoid", cot)
    for u, v, t, name in zip(a, w, truth, ("m", "gx", "gmask_std")):
        check_close(u, v.cpu().numpy(), None, None, what="std/hub/H%d/chunk32-vs-whole/%s" % (H, name), signed_sum=True, truth=t)


# ---- 4: dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,graph,chunk", [(20, "boundary", 512), (128, "hub", 32), (6, "hub", 32)])
def test_explicit_keep_mask(H, graph, chunk):
    from mma_amd import functional as Fn
    add_all = _BOUNDARY if graph == "boundary" else _HUB
    E = sum(len(a) for a in add_all)
    keep = torch.from_numpy((np.random.default_rng(5).random((1, E, H)) >= 0.5).astype(np.uint8))
    layer = make_layer(add_all, H, ["std"], "sigmoid", 0.5, chunk=chunk)
    layer.drop_override = Fn.DropoutSpec(0.5, keep=keep.to(DEV))
    x, cot = inputs(add_all, H)
    # with dropout a degree >= 2 target may keep one message or none in a column: exact arithmetic on both sides (0, or v^2/d - (v/d)^2)
    got = run_std(layer, x, cot)
    compare(got, x, layer.mask_std.detach().cpu(), add_all, "sigmoid", cot, "std/keep/%s/H%d" % (graph, H), keep=keep[0], p=0.5)


def test_explicit_keep_slice_by_position():
    """An explicit (K,E,H) mask hands std the slice at its position in the aggregator list, the other masks theirs."""
    from mma_amd import functional as Fn
    H = 20
    E = sum(len(a) for a in _BOUNDARY)
    keep = torch.from_numpy((np.random.default_rng(6).random((3, E, H)) >= 0.5).astype(np.uint8))
    layer = make_layer(_BOUNDARY, H, ["mean", "std", "max"], "sigmoid", 0.5, chunk=512)
    x, _ = inputs(_BOUNDARY, H)
    layer.drop_override = Fn.DropoutSpec(0.5, keep=keep.to(DEV))
    with torch.no_grad():
        ms = layer._aggregate_all(["mean", "std", "max"], x.to(DEV))
        alone = make_layer(_BOUNDARY, H, ["mean", "max"], "sigmoid", 0.5, chunk=512)
        for n in ("mean", "max"):
            getattr(alone, "mask_" + n).copy_(getattr(layer, "mask_" + n))
        alone.drop_override = Fn.DropoutSpec(0.5, keep=keep[[0, 2]].contiguous().to(DEV))
        rest = alone._aggregate_all(["mean", "max"], x.to(DEV))
    assert ms.shape == (3, len(_BOUNDARY), H) and torch.equal(ms[0], rest[0]) and torch.equal(ms[2], rest[1])
    W = layer.mask_std.detach().cpu()
    want = std_oracle(x, W, _BOUNDARY, "sigmoid", keep[1], 0.5).numpy()
    truth = std_oracle(x.double(), W.double(), _BOUNDARY, "sigmoid", keep[1], 0.5).numpy()
    check_close(ms[1], want, None, None, what="std/keep/slice", signed_sum=True, truth=truth)


@pytest.mark.parametrize("H,p", [(128, 0.5), (6, 0.5), (20, 0.3)])            # 0.3: a threshold that is no multiple of 256 (16-bit form)
def test_hash_dropout_is_repeatable_and_seeded(H, p):
    from mma_amd import functional as Fn
    layer = make_layer(_HUB, H, ["std"], "sigmoid", p, chunk=32)
    x, cot = inputs(_HUB, H)
    layer.drop_override = Fn.DropoutSpec(p, seed=0x1234567890ABCDEF)
    a, b = run_std(layer, x, cot), run_std(layer, x, cot)
    for u, v in zip(a, b):
        assert torch.equal(u, v) and bool(torch.isfinite(u).all())
    layer.drop_override = Fn.DropoutSpec(p, seed=0x1234567890ABCDF0)
    c = run_std(layer, x, cot)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # the keep rate the forward saw: with p the mean of mu^2 shrinks; a crude sanity check that bits are drawn at all
    layer.drop_override = Fn.DropoutSpec(0.0)
    none = run_std(layer, x, cot)
    assert not torch.equal(a[0], none[0])


def test_p_zero_is_drop_none():
    from mma_amd import functional as Fn
    H = 20
    layer = make_layer(_BOUNDARY, H, ["std"], "sigmoid", 0.0, chunk=512)
    x, cot = inputs(_BOUNDARY, H)
    base = run_std(layer, x, cot)                         # the layer's own DropoutSpec(0.0)
    none = Fn.DropoutSpec(0.0)
    assert none.mode == Fn.DROP_NONE
    layer.drop_override = none
    for u, v in zip(base, run_std(layer, x, cot)):
        assert torch.equal(u, v)
    # the C ABI's other spelling of "no dropout": HASH with threshold 0 (P(drop) = 0 / 65536, scale 1), through the functional API
    hash0 = Fn.DropoutSpec(0.5, seed=77)
    hash0.thr = 0
    graph, W = layer.graph(torch.device(DEV)), layer.mask_std.detach()

    def run(drop):
        xg = x.to(DEV).requires_grad_(True)
        P, Q = (xg @ W[:H]), (xg @ W[H:])
        m = Fn.nc_std_aggregate(xg, P, Q, graph, Fn.ACT_SIGMOID, drop)
        return (m.detach(),) + torch.autograd.grad((m * cot.to(DEV)).sum(), [xg])

    for u, v in zip(run(none), run(hash0)):
        assert torch.equal(u, v)


# ---- 5: degenerate variance, enumerated by construction ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [20, 6])
def test_degenerate_variance(H):
    # target 0: no neighbour; target 1: one neighbour; target 2: two edges from the SAME source (exact variance 0; fp32 may round
    # either way); targets 3..: ordinary
    rng = np.random.default_rng(2)
    N = 40
    add_all = [[], [5], [7, 7]] + [sorted(rng.choice(np.arange(3, N), size=rng.integers(2, 6), replace=False).tolist()) for _ in range(3, N)]
    assert degenerate_targets(add_all) == [0, 1, 2]
    layer = make_layer(add_all, H, ["std"], "sigmoid", 0.0)
    x, _ = inputs(add_all, H)
    g = torch.from_numpy(np.random.default_rng(4).standard_normal((N, H)).astype(np.float32))

    def grads(rows):
        cot = torch.zeros(N, H)
        cot[rows] = g[rows]
        return run_std(layer, x, cot)

    m, gx, gw = grads([0, 1])
    assert float((m[:2] - SQRT_EPS).abs().max()) <= 1e-6
    assert float(gx.abs().max()) == 0.0 and float(gw.abs().max()) == 0.0            # relu' is 0 at 0: exactly no gradient
    m, gx, gw = grads([2])
    assert float((m[2] - SQRT_EPS).abs().max()) <= 1e-4
    bound = 1e-3 * float(g[2].abs().max())
    print("degenerate/H%d: |m - sqrt(eps)| %.3g, max |gx| %.3g, max |gmask| %.3g, bound %.3g" % (
        H, float((m[2] - SQRT_EPS).abs().max()), float(gx.abs().max()), float(gw.abs().max()), bound))
    assert float(gx.abs().max()) <= bound and float(gw.abs().max()) <= bound
    # and the ordinary targets of the same graph against the oracle (cotangent zero on the three above)
    x, cot = inputs(add_all, H)
    compare(run_std(layer, x, cot), x, layer.mask_std.detach().cpu(), add_all, "sigmoid", cot, "std/degenerate-graph/H%d" % H)


# ---- 6: through the layer -----------------------------------------------------------------------------------------------------------------
def test_layer_forward_adds_the_std_tail():
    H = 20
    add_all = small_graph()
    N = len(add_all)
    A64, adj = normalized_adj(add_all)
    full = make_layer(add_all, H, ["mean", "std", "max"], "sigmoid", 0.0)
    part = make_layer(add_all, H, ["mean", "max"], "sigmoid", 0.0)
    with torch.no_grad():
        for n in ("mean", "max"):
            getattr(part, "mask_" + n).copy_(getattr(full, "mask_" + n))
        part.weight.copy_(full.weight); part.bias.copy_(full.bias)
    x, _ = inputs(add_all, H)
    cot = torch.from_numpy(np.random.default_rng(8).standard_normal((N, C_OUT)).astype(np.float32))
    xg = x.to(DEV)
    full.mask_std.grad = None
    out = full(xg, adj)
    gstd, = torch.autograd.grad((out * cot.to(DEV)).sum(), [full.mask_std])
    with torch.no_grad():
        diff = out.detach() - part(xg, adj)
    factor = full._scaler_factor(N, torch.device(DEV)).detach().cpu().reshape(-1, 1)        # the scaler stage: a row factor on m W
    Wm, Wo = full.mask_std.detach().cpu(), full.weight.detach().cpu()

    def tail(dtype):
        W = Wm.to(dtype).requires_grad_(True)
        m = std_oracle(x.to(dtype), W, add_all, "sigmoid")
        t = A64.to(dtype) @ (factor.to(dtype) * (m @ Wo.to(dtype)))
        g, = torch.autograd.grad((t * cot.to(dtype)).sum(), [W])
        return t.detach().numpy(), g.numpy()

    (t64, g64), (t32, g32) = tail(torch.float64), tail(torch.float32)
    print("layer: max |diff - fp64 tail| %.3g, max |gmask - fp64| %.3g" % (
        np.abs(diff.cpu().numpy() - t64).max(), np.abs(gstd.cpu().numpy() - g64).max()))
    check_close(diff, t32, None, None, what="std/layer/tail", signed_sum=True, truth=t64)
    check_close(gstd, g32, None, None, what="std/layer/gmask_std", signed_sum=True, truth=g64)


def test_layer_with_std_alone_trains_a_step():
    H = 20
    add_all = small_graph()
    _, adj = normalized_adj(add_all)
    layer = make_layer(add_all, H, ["std"], "new_sigmoid", 0.5)
    x, _ = inputs(add_all, H)
    params = [layer.mask_std, layer.weight, layer.bias]
    opt = torch.optim.SGD(params, lr=0.1)
    before = [p.detach().clone() for p in params]
    out = layer(x.to(DEV), adj)
    assert out.shape == (len(add_all), C_OUT)
    out.square().mean().backward()
    opt.step()
    for p, b in zip(params, before):
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(p.grad).all()) and not torch.equal(p.detach(), b)
    assert bool(torch.isfinite(layer(x.to(DEV), adj)).all())


# ---- 7: surface ---------------------------------------------------------------------------------------------------------------------------
def test_strict_mode_and_the_other_unusable_aggregators_still_raise():
    H = 8
    add_all = small_graph(30)
    _, adj = normalized_adj(add_all)
    x = inputs(add_all, H)[0].to(DEV)
    strict = make_layer(add_all, H, ["std"], strict_reference=True)
    with pytest.raises(NotImplementedError):
        strict.learnable_std(x, None)
    with pytest.raises(NotImplementedError):
        strict(x, adj)
    for name in ("normalized_mean", "moment_3"):
        for mode in (True, False):
            layer = make_layer(add_all, H, [name], strict_reference=mode)
            with pytest.raises(NotImplementedError):
                getattr(layer, "learnable_" + name)(x, None)
            with pytest.raises(NotImplementedError):
                layer(x, adj)
    assert make_layer(add_all, H, ["std"]).learnable_std(x, None).shape == (len(add_all), H)


def test_graph_capture_replays_with_fresh_std_dropout_bits():
    H = 20
    add_all = small_graph()
    _, adj = normalized_adj(add_all)
    layer = make_layer(add_all, H, ["mean", "std"], "sigmoid", 0.5)
    layer.graph_capturable = True
    x = inputs(add_all, H)[0].to(DEV).requires_grad_(True)
    cot = torch.randn(len(add_all), C_OUT, device=DEV)

    def step():
        x.grad = None
        out = layer(x, adj)
        out.backward(cot)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                       # warm-up: the seed states are drawn, the plans and caches built
            step()
    torch.cuda.current_stream().wait_stream(s)
    assert layer._seeds.n == 2                   # one device seed for the fused group, one for std
    seeds_obj = layer._seeds
    with torch.no_grad():                        # single-aggregator calls share the layer's seed set instead of re-creating it
        layer.learnable_std(x, None)
        layer.learnable_mean(x, None)
    step()
    assert layer._seeds is seeds_obj
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_static = step()
    outs, seeds = [], []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        outs.append((out_static.clone(), x.grad.clone()))
        seeds.append(layer._seed_buf.cpu().tolist())
    assert seeds[0][1] != seeds[1][1] and seeds[0][0] != seeds[0][1]
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])
    assert all(bool(torch.isfinite(t).all()) for o in outs for t in o)


def test_std_refuses_to_share_a_fused_groups_device_seed():
    """std is mask 0 of its own launch: on the fused group's device seed it would draw that group's mask-0 bits."""
    from mma_amd import functional as Fn
    H = 8
    add_all = small_graph(30)
    layer = make_layer(add_all, H, ["mean", "std"], "sigmoid", 0.5)
    x = inputs(add_all, H)[0].to(DEV)
    layer.drop_override = Fn.DropoutSpec(0.5, seed_tensor=torch.zeros(1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="seed of its own"):
        layer._aggregate_all(["mean", "std"], x)
    layer.drop_override = Fn.DropoutSpec(0.5, seed_tensor=torch.arange(2, dtype=torch.int64, device=DEV))
    assert layer._aggregate_all(["mean", "std"], x).shape == (2, len(add_all), H)
