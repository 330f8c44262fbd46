"""The HIP-free decision headers of the host side (csrc/pbn_chain_split.hpp, pbn_step_plan.hpp, pbn_env_plan.hpp) under
host sanitizers, on the CPU. First the slice rule of step mode's launch chains:

``make chainsplitcheck`` compiles tests/host/chain_split_check.cpp (no HIP header, no library, no GPU) with
ASan + UBSan and runs it: for every batch size up to 5,000, 1 / 2 / 4 chains and both step block sizes (and
the bench sizes 2^20 and 2^23) the slices tile the batch in order, start at even envs, are never empty, and
1M envs in two chains give two halves of 2^19.
"""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_chain_split_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", str(ROOT / "gym-pbn-stac_amd"), "chainsplitcheck"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "chain_split_check ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_step_plan_is_clean_under_asan_and_ubsan():
    """``make stepplancheck``: tests/host/step_plan_check.cpp on csrc/pbn_step_plan.hpp, the same way. The batch
    shape and the call plan against a restatement of their rules either side of every size threshold, and the
    power-of-two decomposition of every call length up to 5,000 against the greedy loop it replaced."""
    r = subprocess.run(["make", "-C", str(ROOT / "gym-pbn-stac_amd"), "stepplancheck"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "step_plan_check ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_env_plan_is_clean_under_asan_and_ubsan():
    """``make envplancheck``: tests/host/env_plan_check.cpp on csrc/pbn_env_plan.hpp, the same way. Every field of
    the R6 launch plan, and the occupancy queries it makes in their order, against a restatement of the rule as the
    host files held it, over the layouts of the Bittner networks and tt200 and four synthetic ones, 1 to 12 cubes,
    batch sizes either side of every threshold, per-step and fused calls, replay, and every PBNSIM_ENV_* knob forced;
    no class of plan (each kernel mode, chunk, lane limit, hand-off, grid pool, failed query) is left empty."""
    r = subprocess.run(["make", "-C", str(ROOT / "gym-pbn-stac_amd"), "envplancheck"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "env_plan_check ok" in r.stdout
