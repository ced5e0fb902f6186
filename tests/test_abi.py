"""CPU checks of the drop-in boundary: the ctypes signatures hmmc_amd/_lib.py derives from include/hmmc_hip.h cover every
declaration, and libhmmc_hip.so exports exactly the declared entry points."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_ctypes_signatures_match_header():
    from hmmc_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    names = re.findall(r"\b(hmmc_\w+)\s*\(", src)
    assert len(names) == len(set(names)) == len(_lib.SIGNATURES), sorted(set(names) ^ set(_lib.SIGNATURES))
    assert set(names) == set(_lib.SIGNATURES)
    # pinned signatures guard the parser itself (pointers, long, size_t, const char*, no arguments, non-int returns)
    assert _lib.SIGNATURES["hmmc_gemm_f16"] == ("pppiiiiiiiippppipzp", "i")
    assert _lib.SIGNATURES["hmmc_bn_apply_relu"] == ("pppppplip", "i")
    assert _lib.SIGNATURES["hmmc_set_option"] == ("si", "i")
    assert _lib.SIGNATURES["hmmc_mt_chunk_elems"] == ("", "i")
    assert _lib.SIGNATURES["hmmc_tower_workspace_bytes"] == ("liiii", "z")
    assert _lib.ERRORS == {-1: "invalid argument", -2: "unsupported shape/alignment", -3: "workspace too small",
                           -4: "kernel launch failed"}
    from hmmc_amd import ops
    assert (ops.EPI_BIAS, ops.EPI_RELU, ops.EPI_COLSUM, ops.EPI_ROWSCALE) == (1, 16, 32, 1024) and len(_lib.EPI) == 11


def test_library_builds_and_exports_header_symbols():
    from hmmc_amd import build, _lib
    build.build(verbose=False)
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("hmmc_")}
    assert exported == set(_lib.SIGNATURES), sorted(exported ^ set(_lib.SIGNATURES))


def test_options_and_release_entry_points(monkeypatch):
    """hmmc_set_option / hmmc_get_option / hmmc_tower_release (no GPU needed: settings and an empty event cache), and the
    environment translation of hmmc_amd/_lib.py - the library itself reads no environment variable."""
    from hmmc_amd import _lib
    lib = _lib.load()
    for key in _lib.ENV_OPTIONS.values():
        before = _lib.get_option(key)
        _lib.set_option(key, True)
        assert _lib.get_option(key) is True
        _lib.set_option(key, False)
        assert _lib.get_option(key) is False
        _lib.set_option(key, before)
    assert lib.hmmc_set_option(b"no_such_option", 1) == -1 and lib.hmmc_get_option(b"no_such_option") == -1
    assert lib.hmmc_set_option(None, 1) == -1
    with pytest.raises(KeyError):
        _lib.set_option("nope", 1)
    assert lib.hmmc_tower_release(None, None) == 0           # nothing cached in a process that never ran a tower backward
    # no getenv in the product sources, and none of the removed build-time experiment switches
    import glob
    removed = ("HMMC_SCRATCH", "HMMC_DBG", "HMMC_PHASES", "HMMC_PF", "HMMC_ATTN_SKIP", "HMMC_ATTN_PIN", "HMMC_ATTN_ABL",
               "HMMC_ATTN_FWD_WPB", "HMMC_F32_PICK")
    for src in glob.glob(os.path.join(ROOT, "hmmc_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "hmmc_amd", "csrc", "*.h")):
        text = open(src).read()
        assert "getenv" not in text, src
        assert not [m for m in removed if re.search(rf"\b{m}\b", text)], src
    # a variable that is present - even empty - switches its option on when the library is loaded
    monkeypatch.setenv("HMMC_NO_F32_WAVEK", "")
    monkeypatch.setattr(_lib, "_lib", None)
    try:
        _lib.load()
        assert _lib.get_option("no_f32_wavek") is True
    finally:
        _lib.set_option("no_f32_wavek", False)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from hmmc_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="no CPU or eager fallback"):
        _lib.load()


def test_committed_traffic_record_matches_the_kernel_source_and_the_step_it_was_taken_on():
    """bench.py reports `roofline.traffic` from the newest profiles/r*_gemm_f16_hbm_traffic.json only if the record was taken on
    this gemm_f16.hip and counts the launches of the steps it ran (round 4 shipped a record that divided by one step too many
    after the profiled command lost its trailing step: the bench line would have said `traffic: null`)."""
    import glob, hashlib, json, os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = sorted(glob.glob(os.path.join(root, "profiles", "r*_gemm_f16_hbm_traffic.json")))
    assert paths, "no committed PMC record"
    rec = json.load(open(paths[-1]))
    src = open(os.path.join(root, "hmmc_amd", "csrc", "gemm_f16.hip"), "rb").read()
    assert rec["gemm_f16_hip_sha256_16"] == hashlib.sha256(src).hexdigest()[:16], "re-collect: scratch/collect_traffic.sh"
    m_steps, m_warm = re.search(r"--steps (\d+)", rec["command"]), re.search(r"--warmup (\d+)", rec["command"])
    ran = int(m_steps.group(1)) + int(m_warm.group(1)) + (0 if "--roofline-steps 0" in rec["command"] else 1)
    assert rec["steps_profiled"] == ran, (rec["steps_profiled"], ran)
    assert rec["launches"] == rec["launches_per_step"] * rec["steps_profiled"]
