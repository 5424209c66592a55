"""Flat-import shim: the reference's scripts do `from layers import GraphConvolution, MMA` (models.py:4).

`MMA` here keeps the drop-in constructor - the reference's positional arguments (layers.py:57-61) and the keyword extensions DESIGN.md 1
lists, which tests/test_compat_signatures.py pins.  The storage option `logit_dtype` belongs to the package's own class
(`mma_amd.MMA(..., logit_dtype=torch.bfloat16)`), of which this one is a subclass; a script that imports flat sets it as an attribute
(`layer.logit_dtype = torch.bfloat16`) if it wants it."""
from mma_amd import layers as _layers
from mma_amd.graph import DEFAULT_CHUNK
from mma_amd.layers import GraphConvolution  # noqa: F401


class MMA(_layers.MMA):
    __doc__ = _layers.MMA.__doc__

    def __init__(self, add_all, activation, k, in_features, out_features, weight, bias,
                 weight_moment_3, weight_sum, weight_sum2, weight_sum3, weight_sum4, weight_mean,
                 weight_mean2, weight_mean3, weight_mean4, weight_max, weight_max2, weight_max3,
                 weight_max4, weight_min, weight_min2, weight_min3, weight_min4, weight_softmax,
                 weight_softmin, weight_std, weight_normalized_mean, dropout, aggregator_list, device,
                 chunk=DEFAULT_CHUNK, strict_reference=True, scalers=None, compound_scalers=False, avg_d=None):
        super().__init__(add_all, activation, k, in_features, out_features, weight, bias,
                         weight_moment_3, weight_sum, weight_sum2, weight_sum3, weight_sum4, weight_mean,
                         weight_mean2, weight_mean3, weight_mean4, weight_max, weight_max2, weight_max3,
                         weight_max4, weight_min, weight_min2, weight_min3, weight_min4, weight_softmax,
                         weight_softmin, weight_std, weight_normalized_mean, dropout, aggregator_list, device,
                         chunk=chunk, strict_reference=strict_reference, scalers=scalers, compound_scalers=compound_scalers, avg_d=avg_d)
