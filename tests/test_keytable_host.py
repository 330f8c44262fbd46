"""The find-or-insert walk of the device tables (csrc/pbn_keytable.hpp) on the CPU, under ASan + UBSan
(``make keytablecheck``)."""
import pytest


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ is not installed")
def test_keytable_header_is_clean_under_asan_and_ubsan():
    """``make keytablecheck``: tests/host/keytable_check.cpp on csrc/pbn_keytable.hpp alone (no HIP header, no library,
    no GPU) with ASan + UBSan: the walk reach_find and census_find run, over the reach set's model and bookkeeping,
    against a std::map for W = 1, 2, 5 and 8 -- 3,000 inserts of 40 keys, publish races whose losers' entries end dead
    and on the free ring, the next level taking them before the end of keys, max_states, the end of keys and a full
    table."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    r = subprocess.run(["make", "-C", str(root / "gym-pbn-stac_amd"), "keytablecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "keytable_check ok" in r.stdout
