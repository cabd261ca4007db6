"""Shared pytest configuration.

Markers:
  gpu — needs a real MI355X (run on the GPU box with `pytest -m gpu`).  Everything else runs
        on CPU in the build container.
"""
import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

# Two-pass AA frames (drt_capi.hip plan) are planned for frames of >= 2^23 samples or scenes of
# >= 2^19 objects; the parity tests render small frames and should cover the two-pass path, so they
# force it at every size (DRT_AA_TWO_PASS=2; test_aa_two_pass_size_rule checks the default rule).
os.environ.setdefault("DRT_AA_TWO_PASS", "2")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: requires an MI355X GPU (HIP)")
    config.addinivalue_line("markers", "slow: long-running CPU test")


@pytest.fixture(scope="session")
def oracle_mod():
    from oracle import oracle as O

    O.build()
    return O
