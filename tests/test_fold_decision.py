"""CPU check of the fold decision: hmmc_tower_fold_supported (the library's shape limits, no device state) and the Python policy
on top of it decide, shape for shape, what the formulas that used to be written out in hmmc_amd/functional.py decided."""
import itertools

import pytest

LIMIT = 2**31 - 2**24                          # operands of 2 GiB, less the overreach of a GEMM's last tile


def _edge(D):
    """The first token count whose [T + 256, 4 D] fp16 operand reaches the limit."""
    return -(-LIMIT // (4 * D * 2)) - 256


TOKENS = sorted({1, 210, 511, 512, 1024, 2047, 2048, 4096, 12800, 100000}
                | {_edge(D) + k for D in (768, 1024) for k in (-1, 0, 1)})
WIDTHS = (64, 128, 256, 512, 768, 1024)
LENGTHS = (10, 50, 197, 256, 257)


@pytest.mark.parametrize("no_wgrad_group", [False, True])
def test_fold_decisions_equal_the_written_out_formulas(no_wgrad_group, monkeypatch):
    from hmmc_amd import _lib
    from hmmc_amd import functional as Fn
    lib = _lib.load()
    monkeypatch.setattr(Fn, "_FOLD_LN_TRAIN", "vit")
    before = _lib.get_option("no_wgrad_group")
    _lib.set_option("no_wgrad_group", no_wgrad_group)
    try:
        for T, D, L in itertools.product(TOKENS, WIDTHS, LENGTHS):
            below_2gib = (T + 256) * 4 * D * 2 < 2**31 - 2**24
            train = L <= 256 and D % 256 == 0 and T >= 2048 and (T + 256) * 4 * D * 2 < 2**31 - 2**24 and not no_wgrad_group
            assert Fn.fold_train_enabled(True, T, D, L) == train, (T, D, L)
            assert not Fn.fold_train_enabled(False, T, D, L), (T, D, L)            # "vit": the tower's own default decides
            # the pass that keeps no activations: hmmc_amd/functional.py::_tower_forward asks exactly this
            assert bool(lib.hmmc_tower_fold_supported(T, D, L, 0)) == below_2gib, (T, D, L)
            # capability against policy: the library itself takes training towers from 512 tokens, and differs in nothing else
            capable = L <= 256 and D % 256 == 0 and T >= 512 and below_2gib and not no_wgrad_group
            assert bool(lib.hmmc_tower_fold_supported(T, D, L, 1)) == capable, (T, D, L)
    finally:
        _lib.set_option("no_wgrad_group", before)


def test_fold_switch_values(monkeypatch):
    from hmmc_amd import _lib
    from hmmc_amd import functional as Fn
    _lib.load()
    before = _lib.get_option("no_wgrad_group")
    _lib.set_option("no_wgrad_group", False)         # whatever HMMC_NO_WGRAD_GROUP said when the library was loaded
    try:
        _switch_values(monkeypatch, Fn)
    finally:
        _lib.set_option("no_wgrad_group", before)


def _switch_values(monkeypatch, Fn):
    for value, (default_tower, other_tower) in {"vit": (True, False), "all": (True, True), "1": (True, True), "0": (False, False),
                                                "": (False, False), "off": (False, False)}.items():
        monkeypatch.setattr(Fn, "_FOLD_LN", value)
        monkeypatch.setattr(Fn, "_FOLD_LN_TRAIN", value)
        assert (Fn.fold_enabled(True), Fn.fold_enabled(False)) == (default_tower, other_tower), value
        assert (Fn.fold_train_enabled(True, 4096, 768, 50), Fn.fold_train_enabled(False, 4096, 768, 50)) == (default_tower, other_tower), value
