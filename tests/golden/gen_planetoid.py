#!/usr/bin/env python3
"""The Planetoid files tests/test_ingest.py loads (Cora: graph, features, labels, test index; Pubmed: graph) as plain arrays:
tests/golden/planetoid.npz.  The test writes them back into the Planetoid pickle layout in a temporary directory and runs
mma_amd.utils' loader on it, so no pickle is committed.

    python tests/golden/gen_planetoid.py <directory holding the ind.<dataset>.* files>

Per dataset `d`: d_graph_keys / d_graph_lens / d_graph_nbrs (the dict of lists, keys and neighbour lists in file order);
d_<part>_data / _indices / _indptr / _shape (csr parts x, tx, allx); d_<part> (dense parts y, ty, ally); d_test_index."""
import os
import pickle
import sys

import numpy as np
import scipy.sparse as sp

PARTS = {"cora": ("graph", "x", "y", "tx", "ty", "allx", "ally", "test.index"), "pubmed": ("graph",)}


def main(src):
    out = {}
    for ds, parts in PARTS.items():
        for part in parts:
            path = os.path.join(src, "ind.%s.%s" % (ds, part))
            if part == "test.index":
                out["%s_test_index" % ds] = np.loadtxt(path, dtype=np.int64)
                continue
            with open(path, "rb") as f:
                o = pickle.load(f, encoding="latin1")
            key = "%s_%s" % (ds, part)
            if isinstance(o, dict):
                out[key + "_keys"] = np.asarray(list(o.keys()), dtype=np.int64)
                out[key + "_lens"] = np.asarray([len(v) for v in o.values()], dtype=np.int64)
                out[key + "_nbrs"] = np.asarray([u for v in o.values() for u in v], dtype=np.int64)
            elif sp.issparse(o):
                o = o.tocsr()
                out.update({key + "_data": o.data, key + "_indices": o.indices, key + "_indptr": o.indptr,
                            key + "_shape": np.asarray(o.shape, dtype=np.int64)})
            else:
                out[key] = np.asarray(o)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "planetoid.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
