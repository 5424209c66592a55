"""The host prologue of K3 / K4 (mma_gr_fused_fwd / mma_gr_fused_bwd), with no GPU: every call fails a check or returns before a
launch.  Device pointers are None (NULL) throughout; the one exception is the row-maxima pair check, which no set of NULLs can
fail - its case hands over a real one-element host tensor, which the check refuses before anything could read it.  The cases walk
the checks in the order the entry points make them: each case satisfies everything ahead of the message it expects."""
import pytest
import torch

from mma_amd import _lib

SUM, MEAN, MIN, MAX, VAR, STD = range(6)       # aggregator codes of gr_fused.hip
IDENTITY, INVERSE_LINEAR = 0, 4                # first and last scaler code
MAX_K = 8                                      # MMA_MAX_K


def gr_args(name, **kw):
    """Positional arguments of `name`: all pointers NULL, a valid shape and valid codes, then `kw` by parameter name."""
    a = dict(rowptr=None, src=None, perm=None, U=None, V=None, lduv=0, Z=None, ldz=0, by_pos=0, z_index=None, inputs=None, ldi=0,
             amin8=None, amax8=None, amin_side=None, amax_side=None, mean=None, var=None, ldsave=0, long_nodes=None,
             N=1, E=1, T=1, F=4, aggr_host=[SUM, MAX], K=2, scaler_host=[IDENTITY], S=1, avg_log=1.0, avg_lin=1.0,
             drop_mode=0, drop_thr=0, seed=0, seed_dev=None, stream=_lib.STREAM)
    if name == "mma_gr_fused_fwd":
        a.update(out=None)
    else:
        a.update(gout=None, gmsg=None, ldg=0, gU=None, ldgu=0, gmsg_row_max=None, gu_row_max=None)
    unknown = set(kw) - set(a)
    assert not unknown, unknown
    a.update(kw)
    names = [n for _, _, n in _lib._abi.FUNCTIONS[name][1]]
    assert sorted(names) == sorted(a), (names, sorted(a))
    return [a[n] for n in names]


def refused(name, message, **kw):
    with pytest.raises(_lib.MMALibraryError) as e:
        _lib.call(name, *gr_args(name, **kw))
    assert message in str(e.value), str(e.value)


ENTRY_POINTS = ["mma_gr_fused_fwd", "mma_gr_fused_bwd"]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_gr_prologue_checks_fire_in_order(name):
    # 1. the range line, with N, E and T*F each out of range (the codes are bad too: the range line comes first)
    bad_codes = dict(aggr_host=None, scaler_host=None, K=0, S=0)
    refused(name, "N=2147483648 E=1 T=1 F=4 unsupported", N=1 << 31, **bad_codes)
    refused(name, "N=-1 E=1 T=1 F=4 unsupported", N=-1, **bad_codes)
    refused(name, "N=1 E=2147483648 T=1 F=4 unsupported", E=1 << 31, **bad_codes)
    refused(name, "N=1 E=-1 T=1 F=4 unsupported", E=-1, **bad_codes)
    refused(name, "N=1 E=1 T=4096 F=4096 unsupported", T=4096, F=4096, **bad_codes)
    refused(name, "N=1 E=1 T=0 F=4 unsupported", T=0, **bad_codes)
    # 2. K / S, ahead of the NULL lists
    refused(name, "K=0 (1..%d) / S=1 (1..8) unsupported" % MAX_K, K=0, aggr_host=None, scaler_host=None)
    refused(name, "K=%d (1..%d) / S=1 (1..8) unsupported" % (MAX_K + 1, MAX_K), K=MAX_K + 1, aggr_host=None, scaler_host=None)
    refused(name, "K=2 (1..%d) / S=9 (1..8) unsupported" % MAX_K, S=9, aggr_host=None, scaler_host=None)
    # 3. the code lists, ahead of their contents
    refused(name, "NULL aggregator / scaler code list", aggr_host=None, scaler_host=[9])
    refused(name, "NULL aggregator / scaler code list", aggr_host=[9, 9], scaler_host=None)
    # 4. aggregator codes ahead of scaler codes
    refused(name, "aggregator code 6 unknown", aggr_host=[STD, STD + 1], scaler_host=[INVERSE_LINEAR + 1])
    refused(name, "scaler code 5 unknown", aggr_host=[VAR, STD], scaler_host=[INVERSE_LINEAR + 1])


def test_gr_bwd_row_maxima_come_as_a_pair():
    # after the codes, ahead of the N == 0 / E == 0 return and of the NULL line.  One real host word: never read
    word = torch.zeros(1)
    for kw in (dict(gmsg_row_max=word), dict(gu_row_max=word), dict(gmsg_row_max=word, gu_row_max=word)):     # the last: no gU
        refused("mma_gr_fused_bwd", "the row maxima come as a pair", N=0, **kw)
        refused("mma_gr_fused_bwd", "the row maxima come as a pair", **kw)
    refused("mma_gr_fused_bwd", "scaler code 5 unknown", gmsg_row_max=word, scaler_host=[5])                  # the codes come first


def test_gr_empty_calls_return_before_anything_is_dereferenced():
    _lib.call("mma_gr_fused_fwd", *gr_args("mma_gr_fused_fwd", N=0, E=0))
    _lib.call("mma_gr_fused_fwd", *gr_args("mma_gr_fused_fwd", N=0, E=5))
    _lib.call("mma_gr_fused_bwd", *gr_args("mma_gr_fused_bwd", N=0, E=0))
    _lib.call("mma_gr_fused_bwd", *gr_args("mma_gr_fused_bwd", N=0, E=5))
    _lib.call("mma_gr_fused_bwd", *gr_args("mma_gr_fused_bwd", N=3, E=0))
    # ... but not before the codes are checked
    refused("mma_gr_fused_fwd", "aggregator code 7 unknown", N=0, aggr_host=[7, 0])
    refused("mma_gr_fused_bwd", "aggregator code 7 unknown", N=3, E=0, aggr_host=[7, 0])


def test_gr_null_arguments_are_refused_at_one_node_one_edge():
    refused("mma_gr_fused_fwd", "NULL argument", N=1, E=1)
    refused("mma_gr_fused_bwd", "NULL argument or pitch too small", N=1, E=1)
    refused("mma_gr_fused_fwd", "NULL argument", N=1, E=0)            # the forward runs at E == 0: its empty targets get results
