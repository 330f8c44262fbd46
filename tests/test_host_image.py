"""The image packers (csrc/pbn_image.cpp) under host sanitizers, on the CPU.

``make imagecheck`` compiles tests/host/image_check.cpp together with pbn_image.cpp (no HIP header, no
library, no GPU) with ASan + UBSan and runs it: layouts, threshold edge cases, the LDS budget's edge
and the env-config images are checked there against rules stated from the descriptors.
"""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_packers_are_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", str(ROOT / "gym-pbn-stac_amd"), "imagecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "image_check ok" in r.stdout
