"""Which split-precision GEMM a product runs on: dense.nn_form / dense.tn_form against LITERAL tables, on both sides of every
boundary of the decision tree.  The tables were derived from the dispatcher these selectors replaced (gemm_bf16x3's four-way branch,
gemm_f16x2_n128, rows_mm_add_scaled_, _x3_ok, _x3_tn_ok, xt_g, xt_g_batched as they stood before), not from the selectors: a changed
gate shows up here as a changed letter.  Pure integer logic - no GPU; the TN window asks the built library's host-side size queries."""
import pytest

from mma_amd import dense

CODE = {"k": "f16x2_k", "P": "f16x2_k256p", "p": "f16x2_k256", "L": "f16x2_nlp", "n": "f16x2_n128", "6": "bf16x3", "B": "bf16x3_blocks",
        ".": "lib"}
KS = (64, 96, 128, 192, 256, 384, 512, 1024)                    # one word of a table row per K ...
NS = (32, 96, 128, 256, 384, 512, 640, 4096, 4224)              # ... one letter of the word per N
NONE = " ".join(["........."] * 8)
SIX = "......... ......... 666666666 ......... 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB"       # the six-product kernel wherever it is admitted
FWD = "......... ......... 66kkkkkk6 ......... 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB"       # ... and the whole-row kernel at K = 128

# (switches, M, accumulate, row_max_known) -> forms of the entry points (mm_into / _MM / rows_mm_add_ with and without row maxima)
ENTRIES = {
    ("", 4095, False, False): NONE, ("", 4095, True, False): NONE, ("", 4095, True, True): NONE,
    ("", 4096, False, False): FWD, ("", 4096, True, False): SIX, ("", 4096, True, True): SIX,
    ("", 65535, False, False): FWD, ("", 65535, True, False): SIX, ("", 65535, True, True): SIX,
    ("", 65536, False, False): "......... ......... 66kkkkkk6 ......... 666PPPPPn 666Lnnnnn 666Lnnnnn 666Lnnnnn",
    ("", 65536, True, False): SIX,
    ("", 65536, True, True): "......... ......... 666666666 ..nnnn... 66LLnnBBB 66LLnnBBB 66LLnnBBB 66LLnnBBB",
    ("USE_F16X2", 4096, False, False): SIX, ("USE_F16X2", 65536, False, False): SIX, ("USE_F16X2", 65536, True, True): SIX,
    ("USE_NLP", 65535, False, False): FWD,
    ("USE_NLP", 65536, False, False): "......... ......... 66kkkkkk6 ......... 666PPPPPn 666nnnnnn 666nnnnnn 666nnnnnn",
    ("USE_NLP", 65536, True, True): "......... ......... 666666666 ..nnnn... 66nnnnBBB 66nnnnBBB 66nnnnBBB 66nnnnBBB",
    ("PACK_K256", 65535, False, False): FWD,
    ("PACK_K256", 65536, False, False): "......... ......... 66kkkkkk6 ......... 666pppppn 666Lnnnnn 666Lnnnnn 666Lnnnnn",
    ("PACK_K256", 65536, True, True): "......... ......... 666666666 ..nnnn... 66LLnnBBB 66LLnnBBB 66LLnnBBB 66LLnnBBB",
    # bench.py sets _MIN_ROWS_X3 = 1 around its small measurements: the admission moves, the 65536-row gates do not
    ("_MIN_ROWS_X3", 1, False, False): FWD, ("_MIN_ROWS_X3", 4095, False, False): FWD, ("_MIN_ROWS_X3", 4095, True, False): SIX,
    ("_MIN_ROWS_X3", 4095, True, True): SIX, ("_MIN_ROWS_X3", 65535, True, True): SIX,
    ("_MIN_ROWS_X3", 65536, False, False): "......... ......... 66kkkkkk6 ......... 666PPPPPn 666Lnnnnn 666Lnnnnn 666Lnnnnn",
    ("_MIN_ROWS_X3", 65536, True, True): "......... ......... 666666666 ..nnnn... 66LLnnBBB 66LLnnBBB 66LLnnBBB 66LLnnBBB",
}
# (M, accumulate) -> forms of gemm_bf16x3 called by name: no admission, never the library (K = 64 / 96 is _LinearX3's forward)
NAMED = {
    (100, False): "666BBBBBB 666BBBBBB 666666666 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB",
    (4095, False): "666BBBBBB 666BBBBBB 666666666 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB",
    (4096, False): "66kkkkkkB 66kkkkkkB 66kkkkkk6 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB",
    (65535, False): "66kkkkkkB 66kkkkkkB 66kkkkkk6 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB",
    (65536, False): "66kkkkkkB 66kkkkkkB 66kkkkkk6 666nnnnnn 666PPPPPn 666Lnnnnn 666Lnnnnn 666Lnnnnn",
    (65536, True): "666BBBBBB 666BBBBBB 666666666 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB 666BBBBBB",
}


def _flip(monkeypatch, switch):
    if switch == "_MIN_ROWS_X3":
        monkeypatch.setattr(dense, "_MIN_ROWS_X3", 1)
    elif switch:
        assert getattr(dense, switch) is True                    # the defaults the tables assume
        monkeypatch.setattr(dense, switch, False)


def _check(table_row, **kw):
    for K, word in zip(KS, table_row.split()):
        for N, letter in zip(NS, word):
            assert dense.nn_form(kw["M"], K, N, **{k: v for k, v in kw.items() if k != "M"}) == CODE[letter], (kw, K, N)


@pytest.mark.parametrize("key", sorted(ENTRIES), ids=lambda k: "%s-M%d-acc%d-rm%d" % ((k[0] or "default",) + tuple(map(int, k[1:]))))
def test_nn_form_of_the_entry_points(key, monkeypatch):
    switch, M, accumulate, row_max_known = key
    _flip(monkeypatch, switch)
    _check(ENTRIES[key], M=M, accumulate=accumulate, row_max_known=row_max_known)


@pytest.mark.parametrize("key", sorted(NAMED))
def test_nn_form_of_gemm_bf16x3_called_by_name(key):
    _check(NAMED[key], M=key[0], accumulate=key[1], named=True)


def test_nn_form_operands_the_kernels_cannot_take_in_place():
    """`out` with a column stride or another dtype: no three-product form; accumulating into it is the library's.  A misaligned `a`
    with known row maxima: the accumulating three-product kernels read `a` in place, so the six-product kernel (on a copy) runs."""
    _check(SIX, M=65536, accumulate=False, out_ok=False)
    _check(NONE, M=65536, accumulate=True, out_ok=False)
    _check(NONE, M=65536, accumulate=True, row_max_known=True, out_ok=False)
    _check(SIX, M=65536, accumulate=True, row_max_known=True, aligned=False)
    _check("......... ......... 66kkkkkk6 ......... 666PPPPPn 666Lnnnnn 666Lnnnnn 666Lnnnnn", M=65536, accumulate=False, aligned=False)


def test_f16x2_n128_ok_is_the_selectors_answer():
    for M in (65535, 65536):
        for K in KS:
            for N in NS:
                form = dense.nn_form(M, K, N, accumulate=True, row_max_known=True)
                assert dense.f16x2_n128_ok(M, K, N) == (form in ("f16x2_nlp", "f16x2_n128"))
    assert dense.f16x2_n128_ok(65536, 192, 512) and not dense.f16x2_n128_ok(65536, 192, 640) and not dense.f16x2_n128_ok(65536, 128, 128)


# (M, KA, g_row_max_known) -> form of x (M,KA)^T @ g (M,384), dense operands
TN = {
    (1023, 8, False): "lib", (1023, 128, True): "lib", (1023, 256, False): "lib",
    (1024, 7, False): "lib", (1024, 8, False): "bf16x3_tn", (1024, 8, True): "bf16x3_tn", (1024, 128, True): "bf16x3_tn",
    (1024, 129, False): "lib", (1024, 256, False): "bf16x3_tn",
    (65535, 7, True): "lib", (65535, 8, True): "bf16x3_tn", (65535, 128, True): "bf16x3_tn", (65535, 129, True): "lib",
    (65535, 256, True): "bf16x3_tn",
    (65536, 7, True): "lib", (65536, 8, False): "bf16x3_tn", (65536, 8, True): "f16x2_tn", (65536, 128, False): "bf16x3_tn",
    (65536, 128, True): "f16x2_tn", (65536, 129, True): "lib", (65536, 256, False): "bf16x3_tn", (65536, 256, True): "f16x2_tn",
}


@pytest.mark.parametrize("key", sorted(TN))
def test_tn_form(key, monkeypatch):
    M, KA, rm = key
    assert dense.tn_form(M, KA, 384, ldx=KA, ldg=384, g_row_max_known=rm) == TN[key]
    named = dense.tn_form(M, KA, 384, ldx=KA, ldg=384, g_row_max_known=rm, named=True)           # _LinearX3.backward: no admission
    assert named == ("f16x2_tn" if rm and M >= 65536 else "bf16x3_tn")
    monkeypatch.setattr(dense, "USE_F16X2", False)
    assert dense.tn_form(M, KA, 384, ldx=KA, ldg=384, g_row_max_known=rm) == TN[key].replace("f16x2_tn", "bf16x3_tn")


def test_tn_form_thresholds_and_window(monkeypatch):
    # one split's rows through a 32-bit buffer window.  2^20 rows x (128, 1024): 64 splits of 16384 rows -> (16384 + 32) * pitch * 4 < 2^31
    assert dense.tn_form(1 << 20, 128, 1024, ldx=128, ldg=32704, g_row_max_known=True) == "f16x2_tn"
    assert dense.tn_form(1 << 20, 128, 1024, ldx=128, ldg=32705, g_row_max_known=True) == "lib"
    assert dense.tn_form(1 << 20, 128, 1024, ldx=32705, ldg=1024) == "lib"
    assert dense.tn_form(1 << 22, 256, 4096, ldx=256, ldg=4096) == "lib"        # 4 M rows of C5's [gP|gQ]: 8 splits only, 2 GB each
    # batch > 1: one launch from _MIN_ROWS_X3 rows on, 8 <= ka <= 128, nc >= 32, pitch < 2^24, its own window (4 products: 128 splits of
    # 8192 rows); else what one block's product takes
    assert dense.tn_form(1 << 20, 32, 64, ldx=128, ldg=256, batch=4) == "bf16x3_tn_batched"
    assert dense.tn_form(1 << 20, 32, 64, ldx=128, ldg=65280, batch=4) == "bf16x3_tn_batched"
    assert dense.tn_form(1 << 20, 32, 64, ldx=128, ldg=65281, batch=4) == "bf16x3_tn"
    assert dense.tn_form(4096, 32, 64, ldx=128, ldg=256, batch=4) == "bf16x3_tn_batched"
    assert dense.tn_form(4095, 32, 64, ldx=128, ldg=256, batch=4) == "bf16x3_tn"
    assert dense.tn_form(1000, 32, 64, ldx=128, ldg=256, batch=4) == "lib"
    assert dense.tn_form(4096, 32, 31, ldx=128, ldg=124, batch=4) == "bf16x3_tn" and dense.tn_form(4096, 7, 64, ldx=28, ldg=256, batch=4) == "lib"
    assert dense.tn_form(4096, 32, 64, ldx=128, ldg=256, batch=1) == "bf16x3_tn_batched"
    monkeypatch.setattr(dense, "_MIN_ROWS_X3", 1)
    assert dense.tn_form(1000, 32, 64, ldx=128, ldg=256, batch=4) == "bf16x3_tn_batched"
    monkeypatch.setattr(dense, "_MIN_ROWS_TN", 2000)
    assert dense.tn_form(1999, 128, 384, ldx=128, ldg=384) == "lib" and dense.tn_form(2000, 128, 384, ldx=128, ldg=384) == "bf16x3_tn"
    monkeypatch.setattr(dense, "_MIN_COLS_TN", 8)
    assert dense.tn_form(2000, 128, 7, ldx=128, ldg=7) == "lib" and dense.tn_form(2000, 128, 8, ldx=128, ldg=8) == "bf16x3_tn"


def test_tn_columns_per_launch(monkeypatch):
    assert [dense._tn_cols("f16x2_tn", ka) for ka in (8, 75, 128, 256, 384, 512)] == [8, 75, 128, 256, 128, 256]
    assert [dense._tn_cols("bf16x3_tn", ka) for ka in (8, 75, 128, 256, 384, 512)] == [8, 75, 128, 128, 128, 128]
    monkeypatch.setattr(dense, "TN_KA256", False)
    assert [dense._tn_cols("f16x2_tn", ka) for ka in (128, 256, 512)] == [128, 128, 128]


def test_callers_ask_the_selector(monkeypatch):
    """What the callers decide ahead of their GEMMs, at the shapes of the benchmarks: C4 (N = 1 M, H = 128, K = 4 masks), C5 (H = 256,
    K = 8) and the tall Linears of C2L (75 -> 760 on 2e5 rows, 50 -> 380 on 4e5 rows) - and that it is what the entry point then does."""
    # _NCLocalLayer.backward / the sharded layer: a row_max buffer iff rows_mm_add_(gx, [gP|gQ], W^T, row_max) takes a three-product kernel
    for N, H, K in ((1 << 20, 128, 4), (1 << 20, 256, 8)):
        assert dense.f16x2_n128_ok(N, 2 * K * H, H)
        assert dense.nn_form(N, 2 * K * H, H, accumulate=True, row_max_known=True) == "f16x2_nlp"
        assert dense.nn_form(N, 2 * K * H, H, accumulate=True) == ("bf16x3" if H == 128 else "bf16x3_blocks")       # no maxima: six products
    assert dense.nn_form(1 << 20, 128, 1024) == "f16x2_k" and dense.nn_form(1 << 20, 256, 4096) == "f16x2_k256p"      # their forward GEMMs
    assert not dense.f16x2_n128_ok(2708, 2 * 4 * 128, 128)                                                            # Cora: too few rows
    # _LinearX3.forward pads [x | 1] to KP columns; _LinearX3.backward takes dL/dx = g [W | b | 0] (M, OP) x (OP, 128) on the
    # one-accumulator kernel iff the producer of g left its row maxima
    def kp(M, fin, fout):
        k = next(k for k in dense.F16X2_K if fin + 1 <= k)
        return k if dense.nn_form(M, k, dense._round_up(fout, 128), named=True) == "f16x2_k" else 128
    assert kp(200000, 75, 760) == 96 and kp(400000, 50, 380) == 64 and kp(200000, 100, 760) == 128
    assert kp(200000, 75, 4096) == 96 and kp(200000, 75, 4097) == 128 and kp(4000, 75, 760) == 128
    for M, OP in ((200000, 768), (400000, 384)):
        assert dense.f16x2_n128_ok(M, OP, 128) and dense._rows_form(OP, 128) == "f16x2_nlp"
        assert dense.tn_form(M, 96, OP, ldx=96, ldg=OP, g_row_max_known=True, named=True) == "f16x2_tn"
    assert not dense.f16x2_n128_ok(40000, 384, 128)                     # fewer than 65536 rows: gemm_bf16x3(g, wpad[:, :NP])
    assert dense.nn_form(40000, 384, 96, named=True) == "bf16x3"
    monkeypatch.setattr(dense, "USE_NLP", False)
    assert dense.f16x2_n128_ok(200000, 768, 128) and dense._rows_form(768, 128) == "f16x2_n128"
    monkeypatch.setattr(dense, "USE_F16X2", False)
    assert kp(200000, 75, 760) == 128 and not dense.f16x2_n128_ok(200000, 768, 128) and not dense.f16x2_n128_ok(1 << 20, 1024, 128)
    assert dense.tn_form(200000, 96, 768, ldx=96, ldg=768, g_row_max_known=True, named=True) == "bf16x3_tn"


def test_the_callers_hold_no_gates_of_their_own():
    """The predictors call the selector: no row or width threshold of the GEMM dispatch is written out in them."""
    import inspect
    from mma_amd import functional, sharded
    for fn, asks in ((dense._LinearX3.forward, "nn_form("), (dense._LinearX3.backward, "f16x2_n128_ok("),
                     (functional._NCLocalLayer.backward, "f16x2_n128_ok("), (sharded._ShardedAggregate.backward, "f16x2_n128_ok(")):
        src = inspect.getsource(fn)
        assert asks in src
        for gate in ("4096", "1 << 16", "65536", "_MIN_ROWS", "USE_F16X2", "USE_NLP", "PACK_K256"):
            assert gate not in src, (fn.__qualname__, gate)
