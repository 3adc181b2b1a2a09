"""tests/golden/loaded_roadmap_config3_rot.npz is what tests/golden/make_loaded_roadmap.py writes (8 of its rows, recomputed), and holds
what tests/test_gpu_loaded_roadmap.py (test 2) relies on: at least 100 decided candidates, at least 10 of them with a verdict that
differs from the unloaded one.  CPU only: the numpy shooting of tests/loaded_fk_reference.py and the oracle's predicates."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ROWS = np.array([0, 5, 16, 25, 50, 63, 102, 127])      # undecided, decided valid and invalid, verdicts the load moves either way


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "loaded_roadmap_config3_rot.npz")))


def test_generator_reproduces_rows(fx, orc):
    import make_loaded_roadmap as gen
    got = gen.build(rows=ROWS)
    for k in ("states", "valid_loaded", "decided", "valid_unloaded"):
        assert np.array_equal(got[k], fx[k][ROWS]), k
    for k in ("spheres", "grid", "wrench", "dist"):
        assert np.array_equal(got[k], fx[k]), k
    assert np.allclose(got["bound"], fx["bound"][ROWS], rtol=1e-6, atol=0.0)
    dec = fx["decided"][ROWS].astype(bool)
    assert dec.any() and (~dec).any() and (fx["valid_loaded"][ROWS] != fx["valid_unloaded"][ROWS])[dec].any()


def test_counts(fx):
    import make_loaded_roadmap as gen
    dec = fx["decided"].astype(bool)
    assert len(dec) == gen.N_CAND == 128
    assert dec.sum() >= gen.MIN_DECIDED == 100
    moved = (fx["valid_loaded"].astype(bool) != fx["valid_unloaded"].astype(bool)) & dec
    assert moved.sum() >= gen.MIN_MOVED == 10
    voxel = 2 * fx["grid"][1] / fx["grid"][0]
    assert (fx["bound"][dec] <= 0.1 * gen.MARGIN_VOXELS * voxel).all()
    # both verdicts occur among the decided candidates, and a decided candidate is shape-valid by construction
    v = fx["valid_loaded"].astype(bool)[dec]
    assert v.any() and (~v).any()
    print("%d decided (%d valid, %d invalid), %d moved by the load, bound <= %.3g m against %.3g m"
          % (dec.sum(), v.sum(), (~v).sum(), moved.sum(), fx["bound"][dec].max(), gen.MARGIN_VOXELS * voxel))
