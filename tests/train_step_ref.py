"""Plain restatements of the training-step operations (mma_amd/csrc/train_step.hip: K10, K11, K12, K17), written from their formulas,
and the three kinds of bar the tests of those kernels use (tests/test_train_step_kernels_gpu.py).

Every restatement runs in the dtype and on the device of the tensors it is given: float64 on the CPU is the truth, float32 on the GPU is
the yardstick ("what plain torch fp32 ops make of the same formula").  Gradients come from autograd.

  K10  F.log_softmax(x, dim=1) and F.nll_loss(output[idx], labels[idx])            (models.py:68, train.py:77)
  K11  torch.optim.Adam without amsgrad: the recurrence, bias corrections in float64, L2 term folded into the gradient
  K12  (pred - target).abs().mean()                                                (graph_regression/mma.py:156)
  K17  training-mode BatchNorm1d over the first n_valid rows, every row normalised, then ReLU
"""
import math

import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24                                         # unit roundoff of fp32
TINY32 = float(torch.finfo(torch.float32).tiny)            # smallest normal number: the floor of a scale
KBLOCK = 256                                               # threads of the one-workgroup reductions (nll_mean_kernel, l1_mean_kernel)


# ---- K10 --------------------------------------------------------------------------------------------------------------------------
def logsoftmax_nll(x, idx, labels, gloss=1.0):
    """-> (logp (N,C), lse (N), loss, gx (N,C)) in x's dtype / device.  The loss reads the rows idx only, so the gradient is taken
    through x[idx]: a row outside idx gets an exact zero whatever it holds (a NaN row included)."""
    x = x.detach().clone().requires_grad_(True)
    logp = F.log_softmax(x, dim=1)
    loss = F.nll_loss(F.log_softmax(x[idx], dim=1), labels[idx])
    gx, = torch.autograd.grad(loss * gloss, [x])
    return logp.detach(), torch.logsumexp(x.detach(), dim=1), loss.detach(), gx


def nll_from_logp(logp32, idx, labels):
    """The mean the reduction kernel owes for the fp32 log-probabilities it read: (truth in float64, sum of |term|)."""
    rows = idx.cpu()
    terms = -logp32.detach().cpu().double()[rows, labels.cpu()[rows]]
    return terms.sum().item() / rows.numel(), terms.abs().sum().item()


def l1_from_inputs(pred32, target32):
    """(mean |pred - target| in float64 of the fp32 inputs, sum of |d|)."""
    d = (pred32.detach().cpu().double().reshape(-1) - target32.detach().cpu().double().reshape(-1)).abs()
    return d.sum().item() / d.numel(), d.sum().item()


def reduction_bound(n, sum_abs, subtraction=False):
    """One workgroup of 256 threads: a thread adds ceil(n/256) terms in order, then an 8-level tree and one division - at most
    ceil(n/256) + 10 roundings, each at most 2^-24 of the sum of magnitudes; the L1 kernel rounds each difference once more."""
    return (math.ceil(n / KBLOCK) + 10 + (1 if subtraction else 0)) * EPS32 * sum_abs / n


# ---- K12 --------------------------------------------------------------------------------------------------------------------------
def l1_gradient(pred32, target32, gloss, n):
    """fp32, exact: sign(d) * (gloss / n) with the quotient formed in fp32, 0 at ties, NaN where d is NaN."""
    d = pred32.detach().reshape(-1) - target32.detach().reshape(-1)
    scale = torch.tensor(gloss, dtype=torch.float32, device=d.device) / torch.tensor(float(n), dtype=torch.float32, device=d.device)
    return torch.where(d > 0, scale, torch.where(d < 0, -scale, torch.where(d == d, torch.zeros_like(d), d)))


# ---- K11 --------------------------------------------------------------------------------------------------------------------------
class AdamReference:
    """The Adam recurrence in float64 (no amsgrad): g' = g + wd p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""

    def __init__(self, params, betas, eps, weight_decay, step=0, exp_avg=None, exp_avg_sq=None):
        self.p = [p.detach().cpu().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p] if exp_avg is None else [t.detach().cpu().double().clone() for t in exp_avg]
        self.v = [torch.zeros_like(p) for p in self.p] if exp_avg_sq is None else [t.detach().cpu().double().clone() for t in exp_avg_sq]
        self.b1, self.b2 = (float(b) for b in betas)
        self.eps, self.wd, self.t = float(eps), float(weight_decay), int(step)
        self.travel = 0.0                                 # sum of the learning rates taken: k * lr when lr is constant

    def step(self, grads, lr):
        self.t += 1
        self.travel += lr
        bc1, bc2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            g = g.detach().cpu().double() + self.wd * p
            m.mul_(self.b1).add_(g, alpha=1.0 - self.b1)
            v.mul_(self.b2).add_(g * g, alpha=1.0 - self.b2)
            p.sub_(lr / bc1 * m / (v.sqrt() / math.sqrt(bc2) + self.eps))


# ---- K17 --------------------------------------------------------------------------------------------------------------------------
def masked_bn(x, n_valid, gamma, beta, eps, relu, cot, running_mean=None, running_var=None, momentum=0.1):
    """BatchNorm1d (training mode) with the statistics of the first n_valid rows (clamped to 1 .. N), all N rows normalised, then ReLU.
    -> dict(y, gx, ggamma, gbeta, running_mean, running_var); the running variance takes the unbiased estimate, cnt / max(cnt - 1, 1)."""
    N = x.shape[0]
    nv = min(max(int(n_valid), 1), N)
    x = x.detach().clone().requires_grad_(True)
    leaves = [x]
    mean = x[:nv].sum(0) / nv
    var = ((x[:nv] - mean) ** 2).sum(0) / nv
    y = (x - mean) * torch.rsqrt(var + eps)
    if gamma is not None:
        gamma, beta = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
        leaves += [gamma, beta]
        y = y * gamma + beta
    if relu:
        y = torch.relu(y)
    grads = torch.autograd.grad((y * cot).sum(), leaves)
    out = dict(y=y.detach(), gx=grads[0], ggamma=grads[1] if gamma is not None else None, gbeta=grads[2] if gamma is not None else None)
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * running_mean + momentum * mean.detach()
        out["running_var"] = (1 - momentum) * running_var + momentum * var.detach() * (nv / max(nv - 1, 1))
    return out


# ---- the bars ---------------------------------------------------------------------------------------------------------------------
def rel_err(got, truth, scale):
    """max over the elements with a finite truth of |got - truth| / scale.  Where the scale is 0 the value must be exact."""
    truth = truth.detach().cpu().double()
    got = got.detach().cpu().double()
    scale = torch.as_tensor(scale, dtype=torch.float64).cpu().expand_as(truth)
    ok = torch.isfinite(truth)
    if not ok.any():
        return 0.0
    err, sc = (got - truth).abs()[ok], scale[ok]
    q = torch.where(sc > 0, err / sc.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)          # a NaN where the truth is finite is an unbounded error
    return q.max().item()


def assert_within_yardstick(what, kernel, torch32, truth, scale):
    """e_k <= 2 e_t + 4 * 2^-24: the kernel may be twice as far from the float64 truth as torch's fp32 ops are (another summation
    order, another expf), plus four roundings of the scale for the cases torch happens to hit exactly."""
    e_k, e_t = rel_err(kernel, truth, scale), rel_err(torch32, truth, scale)
    print("YARDSTICK %-28s e_k %.3e  e_t %.3e  ratio %.3f" % (what, e_k, e_t, e_k / e_t if e_t > 0 else (0.0 if e_k == 0 else math.inf)))
    assert e_k <= 2.0 * e_t + 4.0 * EPS32, "%s: e_k = %.4e, e_t = %.4e (bar %.4e)" % (what, e_k, e_t, 2.0 * e_t + 4.0 * EPS32)


def assert_same_nans(what, got, truth):
    """NaN exactly where the truth is NaN."""
    assert torch.equal(torch.isnan(got.detach().cpu()), torch.isnan(truth.detach().cpu())), "%s: NaN pattern differs from the float64 truth" % what


def column_scale(truth):
    """Per column: the largest magnitude of the float64 value, floored at the smallest normal fp32 number."""
    t = truth.detach().cpu().double().abs()
    t = torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    return (t.max(0).values if t.dim() == 2 else t).clamp(min=TINY32)
