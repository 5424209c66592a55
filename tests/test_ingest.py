"""Graph ingest: the scipy-only loader must reproduce the reference's networkx-built adjacency.  The
golden fixtures hold the CSR the reference produced for Cora and Pubmed; the Planetoid files the loader reads are
rebuilt in a temporary directory from tests/golden/planetoid.npz (their content as plain arrays, gen_planetoid.py)."""
import collections
import os
import pickle

import numpy as np
import pytest
import scipy.sparse as sp

from golden_util import Golden

PLANETOID = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planetoid.npz")


@pytest.fixture(scope="module")
def DATA(tmp_path_factory):
    """A Planetoid data directory (ind.<dataset>.<part> pickles + ind.cora.test.index) holding the arrays of planetoid.npz."""
    d = tmp_path_factory.mktemp("planetoid")
    z = np.load(PLANETOID)
    (d / "ind.cora.test.index").write_text("".join("%d\n" % i for i in z["cora_test_index"]))
    for ds, part in [("cora", p) for p in ("graph", "x", "y", "tx", "ty", "allx", "ally")] + [("pubmed", "graph")]:
        k = "%s_%s" % (ds, part)
        if part == "graph":                 # a dict of neighbour lists, keys and lists in file order
            nbrs = np.split(z[k + "_nbrs"], np.cumsum(z[k + "_lens"])[:-1])
            obj = collections.defaultdict(list, {int(n): [int(u) for u in v] for n, v in zip(z[k + "_keys"], nbrs)})
        elif part.endswith("x"):            # features: csr matrices
            obj = sp.csr_matrix((z[k + "_data"], z[k + "_indices"], z[k + "_indptr"]), shape=tuple(z[k + "_shape"]))
        else:                               # one-hot labels
            obj = z[k]
        with open(d / ("ind.%s.%s" % (ds, part)), "wb") as f:
            pickle.dump(obj, f)
    return str(d)


@pytest.mark.parametrize("dataset,gold", [("cora", "cora_h64"), ("pubmed", "pubmed_h16")])
def test_loader_reproduces_reference_graph(dataset, gold, DATA):
    from mma_amd.utils import load_graph
    g = Golden(gold)
    adj, add_all = load_graph(dataset, DATA)
    assert adj.shape[0] == g.N and np.array_equal(adj.indptr, g.rowptr) and np.array_equal(adj.indices, g.col)
    assert (adj.data == 1).all() and (adj != adj.T).nnz == 0
    assert all(np.array_equal(a, b) for a, b in zip(add_all[:50], g.add_all[:50]))


def test_load_data_cora_shapes(DATA):
    from mma_amd.utils import load_data
    add_all, adj, features, labels, idx_train, idx_val, idx_test = load_data("cora", DATA)
    assert features.shape == (2708, 1433) and labels.shape == (2708,) and int(labels.max()) == 6
    assert len(add_all) == 2708 and adj.shape == (2708, 2708) and adj._nnz() == 10556
    assert len(idx_train) == 140 + 1068 and len(idx_val) == 500 and len(idx_test) == 1000
