"""The training-step kernels (mma_amd/csrc/train_step.hip: K10 log-softmax + NLL, K11 fused Adam, K12 L1 loss, K17 masked BatchNorm +
ReLU) against float64 restatements (tests/train_step_ref.py) at the edges of their loops: the per-lane column loop of a wavefront, the
4 rows of a workgroup, the strided loops of the one-workgroup reductions, the grid-stride loops, pitched buffers, NULL optional pointers.

Three kinds of bar, none hand-picked:
  * bit-exact where the operation is exact (K12's gradient, zero rows, pad columns, run-to-run equality, the step counter);
  * a derived bound for the two one-workgroup reductions, against the float64 mean of the fp32 values the kernel itself read;
  * everything else against plain torch fp32 on the GPU: e_k <= 2 e_t + 4 * 2^-24, e_k / e_t the kernel's / torch's largest error
    against float64 in units of the quantity's scale (train_step_ref.assert_within_yardstick prints both)."""
import math

import pytest
import torch

import train_step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1234.5678            # what pitched buffers are filled with: a pad column must keep it bit for bit


def _abi(name, *args):
    from mma_amd import _lib
    _lib.call(name, *args, _lib.STREAM)


def _pitched(t, pad):
    """(rows, C + pad) buffer full of the sentinel, t in its first C columns."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), SENTINEL, dtype=torch.float32, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf


def _pads_kept(buf, C):
    return torch.equal(buf[:, C:], torch.full_like(buf[:, C:], SENTINEL))


# ===== K10 =========================================================================================================================
K10_C = [1, 63, 64, 65, 128, 129, 1023, 1024]           # lane loop trips 1, 2, 3, 16 and their edges
K10_N = [1, 3, 4, 5]                                    # a workgroup owns 4 rows


def _logits(N, C, seed, inf_rows=False):
    """5 * randn, and from row 1 on (while there are rows): one row spread over +-80 (the exponentials underflow), one constant row, one
    row whose maximum sits in the last valid column, and with inf_rows one row with a +inf and one that is all -inf."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g) * 5
    kinds = ["spread", "constant", "max_last"] + (["pos_inf", "neg_inf"] if inf_rows else [])
    for r, kind in enumerate(kinds, start=1):
        if r >= N:
            break
        if kind == "spread":
            x[r] = torch.rand(C, generator=g) * 160 - 80
            x[r, 0], x[r, C - 1] = -80.0, 80.0
        elif kind == "constant":
            x[r] = 2.5
        elif kind == "max_last":
            x[r, C - 1] = x[r].max() + 3
        elif kind == "pos_inf":
            x[r, C // 2] = math.inf
        else:
            x[r] = -math.inf
    return x


def _targets(N, C, n_idx, seed):
    """idx: an unsorted sample of a permutation; labels by node, with the classes of the idx rows running down from C - 1 so that every
    class occurs (as far as n_idx goes), column C - 1 first."""
    g = torch.Generator().manual_seed(seed + 1)
    idx = torch.randperm(N, generator=g)[:n_idx]
    if n_idx > 1 and bool((idx[1:] > idx[:-1]).all()):
        idx = idx.flip(0)
    labels = torch.randint(0, C, (N,), generator=g)
    labels[idx] = (C - 1 - torch.arange(n_idx)) % C
    return idx, labels


def _k10_wrapper(x, idx, labels, gloss):
    from mma_amd.train_step import fused_nll_loss
    xd = x.to(DEV).requires_grad_(True)
    loss, logp = fused_nll_loss(xd, idx.to(DEV), labels.to(DEV))
    gx, = torch.autograd.grad(loss * gloss, [xd])
    return logp.detach(), loss.detach(), gx


def _k10_abi(x, idx, labels, gloss, pad, with_loss=True):
    """Through the ABI with ldx = ldo = ldg = C + pad.  -> (logp buffer, loss buffer, gx buffer)"""
    N, C = x.shape
    ld = C + pad
    xb = _pitched(x, pad)
    logp = torch.full((N, ld), SENTINEL, dtype=torch.float32, device=DEV)
    gx = torch.full((N, ld), SENTINEL, dtype=torch.float32, device=DEV)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=DEV)
    idx_d, lab_d = idx.to(DEV), labels.to(DEV)
    _abi("mma_logsoftmax_nll_fwd", xb, ld, idx_d, lab_d, idx.numel(), logp, ld, loss if with_loss else None, N, C)
    _abi("mma_logsoftmax_nll_bwd", logp, ld, idx_d, lab_d, idx.numel(), torch.tensor([gloss], dtype=torch.float32, device=DEV), gx, ld, N, C)
    return logp, loss, gx


def _k10_check(tag, x, idx, labels, gloss, logp, loss, gx):
    N, C = x.shape
    n = idx.numel()
    t_logp, t_lse, t_loss, t_gx = R.logsoftmax_nll(x.double(), idx, labels, gloss)
    y_logp, _, _, y_gx = R.logsoftmax_nll(x.to(DEV), idx.to(DEV), labels.to(DEV), gloss)
    R.assert_same_nans("K10 logp " + tag, logp, t_logp)
    R.assert_same_nans("K10 gx " + tag, gx, t_gx)
    R.assert_within_yardstick("K10 logp [%s]" % tag, logp, y_logp, t_logp, (x.double().abs().max(1).values + t_lse.abs()).unsqueeze(1))
    R.assert_within_yardstick("K10 gx [%s]" % tag, gx, y_gx, t_gx, abs(gloss) / n)
    outside = torch.ones(N, dtype=torch.bool)
    outside[idx] = False
    assert torch.equal(gx.cpu()[outside], torch.zeros(int(outside.sum()), C)), "rows outside idx must be exact zeros"
    want, sum_abs = R.nll_from_logp(logp, idx, labels)               # the mean of the fp32 log-probabilities the kernel read
    if math.isnan(want):
        assert math.isnan(t_loss.item()) and math.isnan(loss.item()), (tag, loss.item())
    else:
        bound = R.reduction_bound(n, sum_abs)
        print("DERIVED   K10 loss [%s] err %.3e bound %.3e" % (tag, abs(loss.item() - want), bound))
        assert abs(loss.item() - want) <= bound, "K10 loss %s: |%.9g - %.9g| = %.3e > %.3e" % (tag, loss.item(), want, abs(loss.item() - want), bound)


@pytest.mark.parametrize("N", K10_N)
@pytest.mark.parametrize("C", K10_C)
def test_k10_shapes(C, N):
    x = _logits(N, C, 100 * C + N)
    idx, labels = _targets(N, C, N, C + N)
    logp, loss, gx = _k10_wrapper(x, idx, labels, 3.0)
    _k10_check("C%d N%d" % (C, N), x, idx, labels, 3.0, logp, loss, gx)
    logp2, loss2, gx2 = _k10_wrapper(x, idx, labels, 3.0)
    assert torch.equal(logp, logp2) and torch.equal(gx, gx2) and torch.equal(loss, loss2), "no atomics: a second call gives the same bits"


@pytest.mark.parametrize("C", K10_C)
def test_k10_special_rows(C):
    """All the row kinds of _logits at every C, the +inf row and the all -inf row among them: NaN where the float64 truth is NaN (these two
    rows, and the loss that reads them), the same values as ever elsewhere."""
    N = 7
    x = _logits(N, C, 7 * C, inf_rows=True)
    idx, labels = _targets(N, C, N, C)
    logp, loss, gx = _k10_wrapper(x, idx, labels, 1.0)
    assert torch.isnan(logp[4:6]).all() and torch.isfinite(logp[[0, 1, 2, 3, 6]]).all()
    _k10_check("C%d special" % C, x, idx, labels, 1.0, logp, loss, gx)
    # the same rows with the two NaN rows outside idx: a finite loss, exact zeros in their gradient rows
    keep = idx[(idx != 4) & (idx != 5)]
    logp, loss, gx = _k10_wrapper(x, keep, labels, 1.0)
    assert torch.isfinite(loss)
    _k10_check("C%d special, finite idx" % C, x, keep, labels, 1.0, logp, loss, gx)


@pytest.mark.parametrize("n_idx", [1, 255, 256, 257, 1000, "N"])
def test_k10_idx_counts(n_idx):
    """The strided loop of nll_mean_kernel: less than one trip, one trip to the element, a second trip, four."""
    N, C = 1003, 7
    n = N if n_idx == "N" else n_idx
    x = _logits(N, C, 11)
    idx, labels = _targets(N, C, n, 3 * n)
    assert n < C or set(labels[idx].tolist()) == set(range(C))
    logp, loss, gx = _k10_wrapper(x, idx, labels, 1.0)
    _k10_check("n_idx %s" % n_idx, x, idx, labels, 1.0, logp, loss, gx)


@pytest.mark.parametrize("gloss", [1.0, 3.0, -2.5, 0.0])
def test_k10_gloss(gloss):
    N, C = 5, 65
    x = _logits(N, C, 21)
    idx, labels = _targets(N, C, 4, 5)
    logp, loss, gx = _k10_wrapper(x, idx, labels, gloss)
    _k10_check("gloss %g" % gloss, x, idx, labels, gloss, logp, loss, gx)


@pytest.mark.parametrize("N,C,n_idx", [(8200, 7, 257), (8200, 65, 8200)], ids=["forward_N8200_C7", "backward_N8200_C65"])
def test_k10_grid_stride_loops(N, C, n_idx):
    """Forward: more than kMaxGrid * 4 = 8192 rows.  Backward: more than kMaxGrid * 256 = 524 288 elements of (n_idx, C)."""
    assert N > 8192 and (n_idx < N or n_idx * C > 524288)
    x = _logits(N, C, N + C)
    idx, labels = _targets(N, C, n_idx, N)
    logp, loss, gx = _k10_wrapper(x, idx, labels, 1.0)
    _k10_check("grid-stride C%d" % C, x, idx, labels, 1.0, logp, loss, gx)


@pytest.mark.parametrize("N,C,n_idx", [(5, 65, 3), (3, 1024, 3), (4, 1, 2), (1003, 7, 257)])
def test_k10_pitched_buffers_through_the_abi(N, C, n_idx):
    """ldx = ldo = ldg = C + 3: the outputs are right, every pad column keeps its sentinel - the zero-fill of the backward included -
    and the pitched call gives the bits of the dense one."""
    x = _logits(N, C, N * C)
    idx, labels = _targets(N, C, n_idx, N + C)
    logp, loss, gx = _k10_abi(x, idx, labels, -2.5, pad=3)
    assert _pads_kept(logp, C), "the forward wrote a pad column of logp"
    assert _pads_kept(gx, C), "the backward (its zero-fill or its kernel) wrote a pad column of gx"
    _k10_check("pitched C%d N%d" % (C, N), x, idx, labels, -2.5, logp[:, :C], loss[0], gx[:, :C])
    logp_d, loss_d, gx_d = _k10_abi(x, idx, labels, -2.5, pad=0)
    assert torch.equal(logp[:, :C], logp_d) and torch.equal(gx[:, :C], gx_d) and torch.equal(loss, loss_d)


def test_k10_without_a_loss_is_a_logsoftmax_only_call():
    """loss = NULL: logp is written as ever and no loss kernel runs - the 1-element loss buffer keeps its sentinel, and the call needs
    neither idx nor labels (a loss launch would have to read them)."""
    N, C = 5, 65
    x = _logits(N, C, 3)
    idx, labels = _targets(N, C, 3, 4)
    logp, loss, _ = _k10_abi(x, idx, labels, 1.0, pad=3, with_loss=False)
    assert loss.item() == torch.tensor(SENTINEL).item(), "the loss buffer keeps its sentinel"
    full, _, _ = _k10_abi(x, idx, labels, 1.0, pad=3)
    assert torch.equal(logp, full) and _pads_kept(logp, C)
    only = torch.full((N, C), SENTINEL, dtype=torch.float32, device=DEV)
    _abi("mma_logsoftmax_nll_fwd", x.to(DEV), C, None, None, 0, only, C, None, N, C)           # no idx, no labels: nothing needs them
    assert torch.equal(only, full[:, :C])


def test_check_targets_on_device_tensors():
    """mma_amd/train_step.py::_check_targets, the host check in front of K10 (it asks torch whether a capture is running, so it needs a
    device): a row outside [0, N), a class outside [0, C), a duplicate row raise what F.nll_loss / indexing would - before any launch."""
    from mma_amd import train_step
    from mma_amd.train_step import fused_nll_loss
    x = torch.randn(6, 5, device=DEV)
    labels = torch.tensor([0, 1, 2, 3, 4, 0])
    for idx, lab, exc, text in [(torch.tensor([0, 6, 2]), labels, IndexError, "index 6 is out of bounds for dimension 0 with size 6"),
                                (torch.tensor([0, -1, 2]), labels, IndexError, "index -1 is out of bounds"),
                                (torch.tensor([0, 1, 2]), torch.tensor([0, 5, 2, 3, 4, 0]), IndexError, "Target 5 is out of bounds"),
                                (torch.tensor([0, 1, 2]), torch.tensor([0, -100, 2, 3, 4, 0]), IndexError, "Target -100 is out of bounds"),
                                (torch.tensor([3, 1, 3]), labels, ValueError, "duplicate rows in idx")]:
        train_step._CHECKED_TARGETS.clear()                 # the verdict is cached per (address, version): never meet a stale one
        with pytest.raises(exc, match=text):
            fused_nll_loss(x, idx.to(DEV), lab.to(DEV))
    train_step._CHECKED_TARGETS.clear()
    fused_nll_loss(x, torch.tensor([5, 0, 3], device=DEV), labels.to(DEV))      # a valid pair passes ...
    assert len(train_step._CHECKED_TARGETS) == 1                                   # ... and is remembered
    train_step._CHECKED_TARGETS.clear()


# ===== K12 =========================================================================================================================
def _l1_case(n, seed, nan_at=None):
    g = torch.Generator().manual_seed(seed)
    pred, y = torch.randn(n, 1, generator=g), torch.randn(n, generator=g)
    y[::7] = pred[::7, 0]                                   # exact ties: gradient 0 there
    if nan_at is not None:
        pred[nan_at, 0] = math.nan
    return pred.to(DEV), y.to(DEV)


def _l1_run_and_check(tag, pred, y, gloss):
    from mma_amd.train_step import fused_l1_loss
    n = y.numel()
    p = pred.clone().requires_grad_(True)
    loss = fused_l1_loss(p.squeeze(-1), y)
    gp, = torch.autograd.grad(loss * gloss, [p])
    assert gp.shape == pred.shape
    want_g = R.l1_gradient(pred, y, gloss, n)
    nan = torch.isnan(want_g)
    assert torch.equal(torch.isnan(gp.view(-1)), nan), "NaN exactly where the difference is NaN"
    assert torch.equal(gp.view(-1)[~nan], want_g[~nan]), "K12's gradient is +-(gloss / n) formed in fp32, 0 at ties: bit for bit"
    ties = torch.arange(0, n, 7, device=DEV)
    assert (gp.view(-1)[ties][~nan[ties]] == 0).all()
    want, sum_abs = R.l1_from_inputs(pred, y)
    if math.isnan(want):
        assert math.isnan(loss.item())
    else:
        bound = R.reduction_bound(n, sum_abs, subtraction=True)
        print("DERIVED   K12 loss [%s] err %.3e bound %.3e" % (tag, abs(loss.item() - want), bound))
        assert abs(loss.item() - want) <= bound, "K12 loss %s: |%.9g - %.9g| = %.3e > %.3e" % (tag, loss.item(), want, abs(loss.item() - want), bound)
    return loss, gp


@pytest.mark.parametrize("gloss", [1.0, 2.5, -1.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 10000])
def test_k12_l1_loss(n, gloss):
    pred, y = _l1_case(n, n)
    a = _l1_run_and_check("n %d gloss %g" % (n, gloss), pred, y, gloss)
    b = _l1_run_and_check("n %d gloss %g again" % (n, gloss), pred, y, gloss)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("n", [1, 257, 10000])
def test_k12_one_nan_in_pred(n):
    """The loss is NaN, the gradient is NaN at that element and +-scale (or 0 at a tie) elsewhere."""
    at = n // 2 if n > 1 else 0
    pred, y = _l1_case(n, n + 1, nan_at=at)
    loss, gp = _l1_run_and_check("n %d NaN" % n, pred, y, 2.5)
    assert math.isnan(loss.item()) and math.isnan(gp[at].item()) and int(torch.isnan(gp).sum()) == 1


def test_k12_grid_stride_loop():
    """600 000 elements: more than kMaxGrid * 256 = 524 288, the backward's grid-stride loop; the forward under its derived bound."""
    pred, y = _l1_case(600000, 6)
    _l1_run_and_check("n 600000", pred, y, 1.0)


# ===== K11 =========================================================================================================================
ADAM_SIZES = [1, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 5]          # chunk edges (4096 elements per workgroup)


def _adam_grads(shapes, steps, seed):
    """Magnitudes spread over 1e-8 .. 1e4 element by element, one in ten an exact zero."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        row = []
        for s in shapes:
            v = torch.randn(s, generator=g) * 10.0 ** (torch.rand(s, generator=g) * 12 - 8)
            v[torch.rand(s, generator=g) < 0.1] = 0.0
            row.append(v)
        out.append(row)
    return out


def _adam_run(cls, init, grads, group_of, lrs, hyper, lr_factor_after=None, loaded=None):
    """group_of[i]: group of tensor i; lrs: one lr per group; lr_factor_after = (k, f): every group's lr is multiplied by f after step k,
    as a scheduler does.  loaded = (step, exp_avg list, exp_avg_sq list) comes in through load_state_dict before the first step."""
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    groups = [{"params": [p for p, gi in zip(ps, group_of) if gi == k], "lr": lr} for k, lr in enumerate(lrs)]
    opt = cls(groups, **hyper)
    if loaded is not None:
        sd = opt.state_dict()
        order = [i for k in range(len(lrs)) for i, gi in enumerate(group_of) if gi == k]          # state ids count through the groups
        sd["state"] = {j: {"step": torch.tensor(float(loaded[0])), "exp_avg": loaded[1][i].clone(), "exp_avg_sq": loaded[2][i].clone()}
                       for j, i in enumerate(order)}
        opt.load_state_dict(sd)
    for p in ps:
        p.grad = torch.zeros_like(p)
    for k, step_g in enumerate(grads):
        if lr_factor_after is not None and k == lr_factor_after[0]:
            for grp in opt.param_groups:
                grp["lr"] *= lr_factor_after[1]
        for p, gg in zip(ps, step_g):
            p.grad.copy_(gg)
        opt.step()
    return ps, opt


def _adam_truth(init, grads, group_of, lrs, hyper, lr_factor_after=None, loaded=None):
    refs = []
    for k, lr0 in enumerate(lrs):
        sel = [i for i, gi in enumerate(group_of) if gi == k]
        ref = R.AdamReference([init[i] for i in sel], hyper["betas"], hyper["eps"], hyper["weight_decay"],
                              **({} if loaded is None else dict(step=loaded[0], exp_avg=[loaded[1][i] for i in sel], exp_avg_sq=[loaded[2][i] for i in sel])))
        lr = lr0
        for s, step_g in enumerate(grads):
            if lr_factor_after is not None and s == lr_factor_after[0]:
                lr *= lr_factor_after[1]
            ref.step([step_g[i] for i in sel], lr)
        refs.append((sel, ref))
    return refs


def _adam_compare(tag, fused, torch_, refs):
    """Parameters in units of |p| + the sum of the learning rates taken (k * lr), moments in units of their tensor's largest magnitude;
    all tensors of the case at once."""
    (fp, fo), (tp, to_) = fused, torch_
    cat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])
    got, yard, truth, scale = {"p": [], "m": [], "v": []}, {"p": [], "m": [], "v": []}, {"p": [], "m": [], "v": []}, {"p": [], "m": [], "v": []}
    for sel, ref in refs:
        for j, i in enumerate(sel):
            for key, state_key, t64 in (("p", None, ref.p[j]), ("m", "exp_avg", ref.m[j]), ("v", "exp_avg_sq", ref.v[j])):
                got[key].append(fp[i] if state_key is None else fo.state[fp[i]][state_key])
                yard[key].append(tp[i] if state_key is None else to_.state[tp[i]][state_key])
                truth[key].append(t64)
                scale[key].append(t64.abs() + ref.travel if key == "p" else torch.full_like(t64, max(t64.abs().max().item(), R.TINY32)))
    for key, name in (("p", "parameters"), ("m", "exp_avg"), ("v", "exp_avg_sq")):
        R.assert_within_yardstick("K11 %s [%s]" % (name, tag), cat(got[key]), cat(yard[key]), cat(truth[key]), cat(scale[key]))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.0, 0.5)], ids=["betas_0.9_0.999", "betas_0_0.5"])
@pytest.mark.parametrize("weight_decay", [0.0, 5e-4], ids=["wd_0", "wd_5e-4"])
def test_k11_adam_against_float64(weight_decay, betas):
    """Six steps, two parameter groups with their own lr, every lr halved after step 3 (the eager path reads group["lr"] per step), tensor
    sizes at the chunk edges, gradients over twelve decades with exact zeros."""
    from mma_amd.train_step import FusedAdam
    g = torch.Generator().manual_seed(17)
    shapes = [(n,) for n in ADAM_SIZES]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = _adam_grads(shapes, 6, 18)
    group_of, lrs = [0, 1, 0, 1, 0, 1, 0], [0.01, 0.003]
    hyper = dict(betas=betas, eps=1e-8, weight_decay=weight_decay)
    fused = _adam_run(FusedAdam, init, grads, group_of, lrs, hyper, lr_factor_after=(3, 0.5))
    torch_ = _adam_run(torch.optim.Adam, init, grads, group_of, lrs, hyper, lr_factor_after=(3, 0.5))
    refs = _adam_truth(init, grads, group_of, lrs, hyper, lr_factor_after=(3, 0.5))
    assert [grp["lr"] for grp in fused[1].param_groups] == [0.005, 0.0015]
    for p in fused[0]:
        assert float(fused[1].state[p]["step"]) == 6.0, "the step counter equals the number of launches"
    _adam_compare("wd %g betas %s" % (weight_decay, betas), fused, torch_, refs)


def test_k11_adam_continues_a_loaded_step_count_of_20000():
    """load_state_dict with step = 20 000: both bias corrections are near 1, and the counter goes on from there."""
    from mma_amd.train_step import FusedAdam
    g = torch.Generator().manual_seed(23)
    shapes = [(4097,), (1,), (33, 7)]
    init = [torch.randn(s, generator=g) for s in shapes]
    m0 = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    v0 = [torch.rand(s, generator=g) * 0.01 for s in shapes]
    grads = _adam_grads(shapes, 4, 24)
    hyper = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
    loaded = (20000, m0, v0)
    fused = _adam_run(FusedAdam, init, grads, [0, 0, 0], [0.01], hyper, loaded=loaded)
    torch_ = _adam_run(torch.optim.Adam, init, grads, [0, 0, 0], [0.01], hyper, loaded=loaded)
    refs = _adam_truth(init, grads, [0, 0, 0], [0.01], hyper, loaded=loaded)
    for p in fused[0]:
        assert float(fused[1].state[p]["step"]) == 20004.0
    assert float(torch_[1].state[torch_[0][0]]["step"]) == 20004.0
    _adam_compare("step 20000", fused, torch_, refs)


@pytest.mark.parametrize("n_tensors,entry", [(120, "mma_adam_step_grads"), (121, "mma_adam_step")], ids=["120_by_value", "121_table"])
def test_k11_adam_at_the_by_value_limit(n_tensors, entry, monkeypatch):
    """Exactly 120 tensors in a group: the gradient pointers travel with the launch (fresh_gradients_ok); 121: the table form."""
    from mma_amd import train_step
    from mma_amd.train_step import FusedAdam
    names = []
    real = train_step.call
    monkeypatch.setattr(train_step, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    g = torch.Generator().manual_seed(n_tensors)
    shapes = [(1 + (7 * i) % 13,) for i in range(n_tensors)]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = _adam_grads(shapes, 3, n_tensors + 1)
    hyper = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
    group_of = [0] * n_tensors
    fused = _adam_run(FusedAdam, init, grads, group_of, [0.01], hyper)
    assert fused[1].fresh_gradients_ok() == (n_tensors <= 120)
    assert names == [entry] * 3, names
    torch_ = _adam_run(torch.optim.Adam, init, grads, group_of, [0.01], hyper)
    assert float(fused[1].state[fused[0][-1]]["step"]) == 3.0
    _adam_compare("%d tensors" % n_tensors, fused, torch_, _adam_truth(init, grads, group_of, [0.01], hyper))


def test_k11_adam_2100_chunks_in_one_launch():
    """One tensor of 2100 * 4096 elements: more workgroups than the chip holds at once, so the last ones start after the first ones have
    finished - and every one of them must still have read the same step count (the ticket scheme).  Against torch.optim.Adam on the GPU
    at the closeness of test_fused_adam_matches_torch_adam."""
    from mma_amd.train_step import FusedAdam
    n = 2100 * 4096
    g = torch.Generator(device=DEV).manual_seed(5)
    init = torch.randn(n, generator=g, device=DEV)
    grads = [torch.randn(n, generator=g, device=DEV) for _ in range(3)]
    res = []
    for cls in (torch.optim.Adam, FusedAdam):
        p = torch.nn.Parameter(init.clone())
        opt = cls([p], lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
        p.grad = torch.zeros_like(p)
        for gg in grads:
            p.grad.copy_(gg)
            opt.step()
        res.append(p.detach())
        step = float(opt.state[p]["step"])
        del opt
    assert step == 3.0
    assert torch.allclose(res[1], res[0], rtol=2e-6, atol=2e-7), (res[1] - res[0]).abs().max().item()


# ===== K17 =========================================================================================================================
BN_N = [1, 63, 64, 65, 511, 512, 513, 1025]             # 64 row lanes, 8 rows in flight per lane: 512 rows per trip
BN_C = [1, 3, 4, 5, 75]                                 # a workgroup owns 4 columns
BN_NV = ["1", "2", "N-1", "N"]
BN_EPS = 1e-5


def _nv(tag, N):
    return {"1": 1, "2": 2, "N-1": N - 1, "N": N, "0": 0, "N+5": N + 5}[tag]


def _bn_inputs(N, C, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return dict(x=offset + torch.randn(N, C, generator=g), gamma=1.0 + 0.5 * torch.randn(C, generator=g), beta=0.5 * torch.randn(C, generator=g),
                cot=torch.randn(N, C, generator=g),          # non-zero on the padded rows too
                rm=torch.randn(C, generator=g), rv=0.5 + torch.rand(C, generator=g))


def _bn_module(C, d, affine=True, track=True):
    bn = torch.nn.BatchNorm1d(C, eps=BN_EPS, affine=affine, track_running_stats=track).to(DEV).train()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"])
        if track:
            bn.running_mean.copy_(d["rm"]); bn.running_var.copy_(d["rv"])
    return bn


def _bn_references(d, nv, affine=True, track=True, relu=True):
    def run(cast):
        gamma, beta = (cast(d["gamma"]), cast(d["beta"])) if affine else (None, None)
        rm, rv = (cast(d["rm"]), cast(d["rv"])) if track else (None, None)
        return R.masked_bn(cast(d["x"]), nv, gamma, beta, BN_EPS, relu, cast(d["cot"]), rm, rv, 0.1)
    return run(lambda t: t.double()), run(lambda t: t.to(DEV))


def _bn_compare(tag, got, truth, yard):
    for key in ("y", "gx", "ggamma", "gbeta", "running_mean", "running_var"):
        if got.get(key) is None:
            continue
        R.assert_within_yardstick("K17 %s [%s]" % (key, tag), got[key], yard[key], truth[key], R.column_scale(truth[key]))


def _bn_wrapper(d, nv, affine=True, track=True):
    from mma_amd import net
    N, C = d["x"].shape
    bn = _bn_module(C, d, affine, track)
    xd = d["x"].to(DEV).requires_grad_(True)
    y = net.masked_bn_relu(xd, bn, torch.tensor(nv, dtype=torch.int64, device=DEV))
    assert type(y.grad_fn).__name__.startswith("_MaskedBNReLU"), "the fused K17 path must have run"
    grads = torch.autograd.grad((y * d["cot"].to(DEV)).sum(), [xd] + ([bn.weight, bn.bias] if affine else []))
    got = dict(y=y.detach(), gx=grads[0], ggamma=grads[1] if affine else None, gbeta=grads[2] if affine else None)
    if track:
        got.update(running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(), tracked=int(bn.num_batches_tracked))
    return got


@pytest.mark.parametrize("nv", BN_NV)
@pytest.mark.parametrize("C", BN_C)
@pytest.mark.parametrize("N", BN_N)
def test_k17_masked_bn_relu(N, C, nv):
    """Forward, all three gradients and the running statistics, cotangent non-zero on the padded rows (the kernel sums g and g * xhat over
    all N rows and applies the mean / variance terms to the first n_valid only: the autograd of the masked formulation)."""
    d = _bn_inputs(N, C, 1000 * N + 10 * C + BN_NV.index(nv))
    n_valid = _nv(nv, N)
    got = _bn_wrapper(d, n_valid)
    truth, yard = _bn_references(d, n_valid)
    assert got["tracked"] == 1, "num_batches_tracked moves by one per call"
    _bn_compare("N%d C%d nv %s" % (N, C, nv), got, truth, yard)


@pytest.mark.parametrize("nv,acts_as", [("0", "1"), ("N+5", "N")])
def test_k17_n_valid_out_of_range_is_clamped(nv, acts_as):
    N, C = 65, 5
    d = _bn_inputs(N, C, 3)
    a, b = _bn_wrapper(d, _nv(nv, N)), _bn_wrapper(d, _nv(acts_as, N))
    for key in ("y", "gx", "ggamma", "gbeta", "running_mean", "running_var"):
        assert torch.equal(a[key], b[key]), key
    truth, yard = _bn_references(d, _nv(nv, N))
    _bn_compare("nv %s" % nv, a, truth, yard)


def test_k17_inputs_far_from_zero():
    """x = 1000 + randn: a one-pass variance (E[x^2] - mean^2) would lose every digit here; the two-pass form holds, and the yardstick
    carries what fp32 inputs cannot avoid (the rounding of a mean near 1000).  75 columns, so that e_k and e_t are each the largest of 75
    independent roundings of a mean, not one against one."""
    N, C = 1025, 75
    d = _bn_inputs(N, C, 77, offset=1000.0)
    got = _bn_wrapper(d, N - 1)
    truth, yard = _bn_references(d, N - 1)
    _bn_compare("1000 + randn", got, truth, yard)


@pytest.mark.parametrize("affine,track", [(False, True), (True, False)], ids=["affine_false", "track_running_stats_false"])
def test_k17_module_options(affine, track):
    """gamma / beta NULL, and the running pointers and the counter NULL, through net.masked_bn_relu."""
    N, C = 513, 5
    d = _bn_inputs(N, C, 5)
    got = _bn_wrapper(d, N - 1, affine, track)
    truth, yard = _bn_references(d, N - 1, affine, track)
    _bn_compare("affine %s track %s" % (affine, track), got, truth, yard)


def _bn_abi(d, nv, relu, pad, param_grads=True):
    N, C = d["x"].shape
    ld = C + pad
    x, gy = _pitched(d["x"], pad), _pitched(d["cot"], pad)
    y = torch.full((N, ld), SENTINEL, dtype=torch.float32, device=DEV)
    gx = torch.full((N, ld), SENTINEL, dtype=torch.float32, device=DEV)
    new = lambda t: t.to(DEV).clone()
    gamma, beta, rm, rv = new(d["gamma"]), new(d["beta"]), new(d["rm"]), new(d["rv"])
    mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    tracked = torch.zeros((), dtype=torch.int64, device=DEV)
    n_valid = torch.tensor(nv, dtype=torch.int64, device=DEV)
    ggamma, gbeta = (torch.empty(C, device=DEV), torch.empty(C, device=DEV)) if param_grads else (None, None)
    _abi("mma_masked_bn_relu_fwd", x, ld, n_valid, gamma, beta, y, ld, mean, rstd, rm, rv, tracked, 0.1, BN_EPS, N, C, relu)
    _abi("mma_masked_bn_relu_bwd", gy, ld, y, ld, x, ld, mean, rstd, gamma, n_valid, gx, ld, ggamma, gbeta, N, C, relu)
    return dict(y=y[:, :C], gx=gx[:, :C], ggamma=ggamma, gbeta=gbeta, running_mean=rm, running_var=rv, tracked=int(tracked)), (y, gx)


@pytest.mark.parametrize("relu,pad,param_grads", [(0, 0, True), (1, 3, True), (0, 3, True), (1, 0, False)],
                         ids=["relu_0", "pitch_C+3", "relu_0_pitch_C+3", "ggamma_gbeta_NULL"])
def test_k17_through_the_abi(relu, pad, param_grads):
    """What only the ABI can say: relu = 0 (plain BatchNorm, forward and backward), row pitches C + 3 on x, y, gy and gx (the pad columns
    of y and gx keep their sentinel), ggamma / gbeta NULL."""
    N, C = 513, 5
    d = _bn_inputs(N, C, 9)
    got, (ybuf, gxbuf) = _bn_abi(d, N - 1, relu, pad, param_grads)
    assert _pads_kept(ybuf, C) and _pads_kept(gxbuf, C)
    assert got["tracked"] == 1
    truth, yard = _bn_references(d, N - 1, relu=bool(relu))
    _bn_compare("relu %d pad %d" % (relu, pad), got, truth, yard)
