"""Ragged batches, the parts that need no GPU: the offsets helper and the argument checks of the four C entries (the C++ adaptor's
ragged model compiling with plain g++: tests/test_cpp_ragged.py)."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def test_ragged_offsets_round_trips_counts():
    from tinyopt_amd import ragged_offsets
    counts = [3, 0, 5, 1, 0]
    off = ragged_offsets(counts=counts)
    assert off.dtype == torch.int64 and off.tolist() == [0, 3, 3, 8, 9, 9]
    assert (off[1:] - off[:-1]).tolist() == counts
    assert torch.equal(ragged_offsets(offsets=off), off) and torch.equal(ragged_offsets(offsets=off.tolist(), total_items=9), off)
    assert torch.equal(ragged_offsets(counts=torch.tensor(counts, dtype=torch.int32)), off)
    assert ragged_offsets(counts=[]).tolist() == [0]


@pytest.mark.parametrize("kw,why", [
    (dict(offsets=[0, 4, 3, 6]), "non-decreasing"),
    (dict(offsets=[1, 4, 6]), r"offsets\[0\]"),
    (dict(counts=[2, 2], total_items=5), "total_items"),
    (dict(offsets=[0, 2, 4], total_items=5), "total_items"),
    (dict(counts=[1], offsets=[0, 1]), "exactly one"),
    (dict(), "exactly one"),
    (dict(counts=[3, -1, 2]), "negative"),
    (dict(counts=[1.5, 2.0]), "integers"),
])
def test_ragged_offsets_says_why_it_refuses(kw, why):
    from tinyopt_amd import ragged_offsets
    with pytest.raises(ValueError, match=why):
        ragged_offsets(**kw)


def test_ragged_entries_refuse_a_null_handle(built):
    from tinyopt_amd import _capi
    lib = _capi.load()
    calls = {
        "toa_jit_lm_run_ragged": (None, None, None, None, 4, 8, 2, None, None, None, None, None, 0),
        "toa_jit_gd_run_ragged": (None, None, None, None, 4, 8, 2, None, None, None, None, None, None, 0),
        "toa_jit_accumulate_ragged": (None, None, None, None, 4, 8, 2, None, None, 1, None, None, None, None),
        "toa_jit_eval_ragged": (None, None, None, None, 4, 8, 2, None, None, None, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == E_ARG, name
        assert name.encode() in lib.toa_last_error() and b"null handle" in lib.toa_last_error()
    assert lib.toa_jit_model_stats_ragged(None, None, None, None, None) == E_ARG
    assert lib.toa_abi_version() == 7   # additive

