"""CPU-side tests (-m "not gpu") of the bf16-output column-group GEMMs (include/mma_amd.h ABI 39: mma_gemm_f16x2_k_h,
mma_gemm_f16x2_k256_h, mma_gemm_f16x2_k256p_h): they are declared with their fp32 twins' parameters, and every bad argument a twin
refuses on the host is refused by its `_h` form with the same text, before any launch - no GPU is needed to see it.  The bf16 form's
own rule (header: the kernels store single 2-byte elements, so C needs 2-byte alignment and any ldc >= N) is checked as well."""
import re

import pytest
import torch

from mma_amd import _lib, dense

M, N = 8, 128
TWINS = [("mma_gemm_f16x2_k", "mma_gemm_f16x2_k_h"), ("mma_gemm_f16x2_k256", "mma_gemm_f16x2_k256_h"),
         ("mma_gemm_f16x2_k256p", "mma_gemm_f16x2_k256p_h")]


def _values(name):
    K = 64 if "_k256" not in name else 256
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    c_dtype = torch.bfloat16 if name.endswith("_h") else torch.float32
    return dict(A=f(M, K), lda=K, Bt2=torch.zeros(2, N, K, dtype=torch.float16), col_unscale=f(N), C=torch.zeros(M, N, dtype=c_dtype), ldc=N,
                a_row_max=None, row_max=f(M), Ap=torch.zeros(32 * 1024, dtype=torch.uint8), sce=torch.zeros(M, dtype=torch.int32),
                M=M, N=N, K=K, stream=None)


def _args(name, **over):
    vals = _values(name)
    vals.update(over)
    return [vals[n] for _, _, n in _lib._abi.FUNCTIONS[name][1]]


def _refusal(name, **over):
    with pytest.raises(_lib.MMALibraryError) as e:
        _lib.call(name, *_args(name, **over))
    return str(e.value).replace(name, "<entry>")


def test_the_abi_is_39_or_later():
    assert _lib.ABI_VERSION >= 39


@pytest.mark.parametrize("f32,h", TWINS)
def test_h_entry_points_are_declared_with_their_twins_parameters(f32, h):
    assert h in _lib._abi.FUNCTIONS and h in _lib.PROTOTYPES
    assert [n for _, _, n in _lib._abi.FUNCTIONS[h][1]] == [n for _, _, n in _lib._abi.FUNCTIONS[f32][1]]
    assert _lib._abi.FUNCTIONS[h] == _lib._abi.FUNCTIONS[f32]          # the bindings see C as a pointer either way


BAD = [
    (dict(N=192), "need N % 128 == 0"),
    (dict(N=64), "need N % 128 == 0"),
    (dict(N=4224, ldc=4224), "N <= 4096"),
    (dict(M=-1), "need N % 128 == 0, N <= 4096"),
    (dict(ldc=N - 1), "row pitch too small"),
    (dict(ldc=1 << 24), "row pitch too small"),
    (dict(C=None), "NULL or misaligned argument"),
    (dict(col_unscale=None), "NULL or misaligned argument"),
    (dict(Bt2=None), "NULL or misaligned argument"),
]


@pytest.mark.parametrize("f32,h", TWINS)
@pytest.mark.parametrize("over,text", BAD, ids=["%d-%s" % (n, "-".join(sorted(o))) for n, (o, _) in enumerate(BAD)])
def test_h_entry_points_refuse_what_their_fp32_twins_refuse(f32, h, over, text):
    want, got = _refusal(f32, **over), _refusal(h, **over)
    assert got == want                                      # the same check, the same text
    assert re.search(text, got), got


def test_k_h_refuses_an_unsupported_reduction_width():
    over = dict(K=80, A=torch.zeros(M, 80), lda=80)
    assert _refusal("mma_gemm_f16x2_k_h", **over) == _refusal("mma_gemm_f16x2_k", **over)
    assert "K=80 unsupported" in _refusal("mma_gemm_f16x2_k_h", **over)


@pytest.mark.parametrize("f32,h", TWINS[:2])
def test_h_entry_points_refuse_the_a_operands_their_twins_refuse(f32, h):
    K = _values(h)["K"]
    for over in (dict(lda=K - 4), dict(lda=K + 2), dict(A=None), dict(A=torch.zeros(M * K + 4)[1:])):       # narrow, unaligned pitch, NULL, 4 bytes off
        assert _refusal(h, **over) == _refusal(f32, **over)


@pytest.mark.parametrize("f32,h", TWINS)
def test_h_entry_points_refuse_an_odd_address_of_c(f32, h):
    """The bf16 form's own alignment rule: 2 bytes (the kernels store single bf16 elements).  One byte off is refused on the host ..."""
    raw = torch.zeros(2 * M * (N + 8) + 2, dtype=torch.uint8)
    assert raw.data_ptr() % 2 == 0
    assert "NULL or misaligned argument" in _refusal(h, C=raw[1:])
    # ... and the fp32 twin refuses a C that is not 4-byte aligned, in the same words
    assert _refusal(f32, C=raw[2:]) == _refusal(h, C=raw[1:])


@pytest.mark.parametrize("f32,h", TWINS)
def test_nothing_to_do_is_no_error(f32, h):
    """M == 0 returns before the pointers are looked at, as in the twins: no launch, no error."""
    assert _lib.call(h, *_args(h, M=0, C=None)) == _lib.call(f32, *_args(f32, M=0, C=None))


def test_gemm_f16x2_takes_float32_and_bfloat16_outputs_only():
    a, w = torch.zeros(4, 64), torch.zeros(64, 128)
    for bad in (torch.float16, torch.float64):
        with pytest.raises(ValueError, match="float32 or bfloat16"):
            dense.gemm_f16x2(a, w, out_dtype=bad)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        dense.gemm_f16x2(a, w, out=torch.zeros(4, 128, dtype=torch.float16))


def test_the_switch_is_on_by_default_and_a_bf16_out_keeps_the_form_of_an_fp32_one():
    import inspect
    assert dense.BF16_EPILOGUE is True or "MMA_BF16_EPILOGUE" in __import__("os").environ
    assert list(inspect.signature(dense.gemm_f16x2).parameters) == ["a", "w", "out", "row_max_out", "out_dtype"]
    assert inspect.signature(dense.gemm_f16x2).parameters["out_dtype"].default == torch.float32
    assert set(dense._BF16_OUT_FORMS) == {"f16x2_k", "f16x2_k256", "f16x2_k256p"} <= set(dense._NN_RUN)
