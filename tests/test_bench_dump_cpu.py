"""bench.py --dump-outputs: what it writes holds the timed path's uint64 proof words and field elements exactly, and stays under its size limit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_dump_is_exact_float64_of_32_bit_halves(tmp_path):
    words = np.array([0, 1, (1 << 64) - 1, 0x0123456789ABCDEF], dtype=np.uint64)
    limbs = np.random.default_rng(1).integers(0, 1 << 63, size=(5, 4), dtype=np.uint64)
    bench.dump_outputs(str(tmp_path / "out"), {"proof_words": words, "limbs": limbs, "small": np.arange(3, dtype=np.float32)})
    got = np.load(tmp_path / "out" / "proof_words.npy")
    assert got.dtype == np.float64 and got.shape == (8,)
    assert (got.astype(np.uint32).view(np.uint64) == words).all()
    got = np.load(tmp_path / "out" / "limbs.npy")
    assert got.shape == (5, 8) and (np.ascontiguousarray(got.astype(np.uint32)).view(np.uint64) == limbs).all()
    assert (np.load(tmp_path / "out" / "small.npy") == np.arange(3)).all()


def test_dump_over_the_limit_is_refused(tmp_path):
    with pytest.raises(SystemExit, match="limit"):
        bench.dump_outputs(str(tmp_path / "out"), {"big": np.zeros(bench.DUMP_LIMIT_BYTES // 16 + 1, dtype=np.uint64)})
    assert not os.path.exists(tmp_path / "out")
