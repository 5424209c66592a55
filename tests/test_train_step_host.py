"""CPU-side tests (-m "not gpu") of the training-step entry points (mma_amd/csrc/train_step.hip: K10, K11, K12, K17, the seed stream):
a valid argument set, one argument made wrong, and the text of the refusal.  Every refusal comes before any launch, so host tensors
stand in for device memory and no GPU is needed to see it (the pattern of tests/test_nc_bf16_host.py).  The Python-side check in front of
K10 (`train_step._check_targets`) asks torch whether a capture is running, which needs a device: its test is in
tests/test_train_step_kernels_gpu.py."""
import re
import struct

import pytest
import torch

from mma_amd import _lib

N, C, NI = 6, 5, 3


def _values():
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    i = lambda *s: torch.zeros(*s, dtype=torch.int64)
    return dict(
        # K10
        x=f(N, C), ldx=C, idx=i(NI), labels=i(N), n_idx=NI, logp=f(N, C), ldo=C, loss=f(1), N=N, C=C, gloss=f(1), gx=f(N, C), ldg=C, stream=None,
        # K12
        pred=f(N), target=f(N), n=N, gpred=f(N),
        # K11: one tensor of one chunk
        table=torch.zeros(_lib.query("mma_adam_table_bytes", 1, 1), dtype=torch.uint8), n_tensors=1, total_chunks=1, step=f(1), lr=0.01,
        beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-4, grad_ptrs_host=list(struct.pack("<Q", 4096)),
        # K17
        n_valid=i(1), gamma=f(C), beta=f(C), y=f(N, C), ldy=C, mean_out=f(C), rstd_out=f(C), running_mean=f(C), running_var=f(C),
        n_tracked=i(1), momentum=0.1, relu=1, gy=f(N, C), mean=f(C), rstd=f(C), ldgx=C, ggamma=f(C), gbeta=f(C),
        # seed stream
        seeds=i(2 * N))


def _refusal(name, **over):
    vals = _values()
    vals.update(over)
    with pytest.raises(_lib.MMALibraryError) as e:
        _lib.call(name, *[vals[n] for _, _, n in _lib._abi.FUNCTIONS[name][1]])
    return str(e.value)


def _passes_without_a_launch(name, **over):
    vals = _values()
    vals.update(over)
    _lib.call(name, *[vals[n] for _, _, n in _lib._abi.FUNCTIONS[name][1]])


NLL_FWD = [
    ("C0", dict(C=0, ldx=1, ldo=1), "C=0 unsupported"),
    ("C1025", dict(C=1025, ldx=1025, ldo=1025), "C=1025 unsupported"),
    ("C1024_passes_the_width_check", dict(C=1024, ldx=1024, ldo=1024, x=None), "NULL argument"),      # refused for what is wrong NEXT
    ("ldx_below_C", dict(ldx=C - 1), "C=%d unsupported" % C),
    ("ldo_below_C", dict(ldo=C - 1), "C=%d unsupported" % C),
    ("N_negative", dict(N=-1), "N=-1 "),
    ("loss_with_n_idx_0", dict(n_idx=0), "the loss needs a non-empty idx and the labels"),
    ("loss_with_NULL_idx", dict(idx=None), "the loss needs a non-empty idx and the labels"),
    ("loss_with_NULL_labels", dict(labels=None), "the loss needs a non-empty idx and the labels"),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in NLL_FWD], ids=[c[0] for c in NLL_FWD])
def test_logsoftmax_nll_fwd_refusals(over, text):
    got = _refusal("mma_logsoftmax_nll_fwd", **over)
    assert text in got and "mma_logsoftmax_nll_fwd failed (code 1)" in got, got


@pytest.mark.parametrize("over,text", [(dict(ldg=C - 1), "C=%d unsupported" % C), (dict(gloss=None), "NULL argument")], ids=["ldg_below_C", "NULL_gloss"])
def test_logsoftmax_nll_bwd_refusals(over, text):
    got = _refusal("mma_logsoftmax_nll_bwd", **over)
    assert text in got and "(code 1)" in got, got


@pytest.mark.parametrize("name", ["mma_l1_loss_fwd", "mma_l1_loss_bwd"])
def test_l1_loss_refuses_an_empty_batch(name):
    got = _refusal(name, n=0)
    assert "n=0: the mean of an empty batch is undefined" in got and "(code 1)" in got, got


ADAM = [
    ("beta1_is_1", dict(beta1=1.0), "invalid Adam hyper-parameters"),
    ("beta2_negative", dict(beta2=-0.5), "invalid Adam hyper-parameters"),
    ("lr_negative", dict(lr=-0.01), "invalid Adam hyper-parameters"),
    ("eps_negative", dict(eps=-1e-8), "invalid Adam hyper-parameters"),
    ("total_chunks_2_to_31", dict(total_chunks=1 << 31), "bad table size"),
]


@pytest.mark.parametrize("name", ["mma_adam_step", "mma_adam_step_grads"])
@pytest.mark.parametrize("over,text", [c[1:] for c in ADAM], ids=[c[0] for c in ADAM])
def test_adam_step_refusals(name, over, text):
    got = _refusal(name, **over)
    assert text in got and "(code 1)" in got, got


def test_adam_size_helpers():
    assert [_lib.query("mma_adam_chunks", n) for n in (0, 1, 4096, 4097)] == [0, 1, 1, 2]
    assert _lib.query("mma_adam_table_bytes", -1, 0) == -1
    assert _lib.query("mma_adam_table_bytes", 2, 3) == 2 * 48 + 3 * 4 + 4            # records | chunk -> tensor ids | ticket
    assert _lib.query("mma_adam_max_grads_by_value") == 120


def _ptr_list(addresses):
    return list(b"".join(struct.pack("<Q", a) for a in addresses))


ADAM_GRADS = [
    ("NULL_pointer_list", dict(grad_ptrs_host=None), "NULL gradient pointer list"),
    ("121_tensors", dict(n_tensors=121, total_chunks=121, table=torch.zeros(121 * 48 + 121 * 4 + 4, dtype=torch.uint8),
                         grad_ptrs_host=_ptr_list([4096] * 121)), "n_tensors=121: at most 120 gradient pointers travel with the launch"),
    ("NULL_gradient_address", dict(grad_ptrs_host=_ptr_list([0])), "gradient 0: NULL or misaligned pointer"),
    ("misaligned_gradient_address", dict(n_tensors=2, total_chunks=2, table=torch.zeros(2 * 48 + 2 * 4 + 4, dtype=torch.uint8),
                                         grad_ptrs_host=_ptr_list([4096, 4098])), "gradient 1: NULL or misaligned pointer"),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in ADAM_GRADS], ids=[c[0] for c in ADAM_GRADS])
def test_adam_step_grads_refusals(over, text):
    got = _refusal("mma_adam_step_grads", **over)
    assert text in got and "(code 1)" in got, got


BN = [
    ("N0", dict(N=0), "N=0 C=%d unsupported" % C),
    ("ldy_below_C", dict(ldy=C - 1), "C=%d unsupported" % C),
]


@pytest.mark.parametrize("name", ["mma_masked_bn_relu_fwd", "mma_masked_bn_relu_bwd"])
@pytest.mark.parametrize("over,text", [c[1:] for c in BN], ids=[c[0] for c in BN])
def test_masked_bn_relu_refusals(name, over, text):
    got = _refusal(name, **over)
    assert text in got and "(code 1)" in got, got


@pytest.mark.parametrize("over,text", [(dict(momentum=1.5), "C=%d unsupported" % C), (dict(running_var=None), "NULL argument"),
                                       (dict(running_mean=None), "NULL argument")],
                         ids=["momentum_above_1", "running_mean_alone", "running_var_alone"])
def test_masked_bn_relu_fwd_refusals(over, text):
    got = _refusal("mma_masked_bn_relu_fwd", **over)
    assert text in got and "(code 1)" in got, got


@pytest.mark.parametrize("n", [-1, (1 << 24) + 1])
def test_seed_advance_refuses_counts_out_of_range(n):
    got = _refusal("mma_seed_advance", n=n)
    assert re.search(r"n=%d out of range" % n, got), got


def test_seed_advance_of_nothing_returns_0():
    _passes_without_a_launch("mma_seed_advance", n=0, seeds=None)                  # return code 0: call() raises on anything else
