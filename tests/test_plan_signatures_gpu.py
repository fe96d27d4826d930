"""The inference plans against the signatures recorded at the commit ``tests/golden/plan_signatures.json`` names (``tools/plan_signatures.py``): every
plan of every case launch for launch - launcher, kernel symbol, flops, bytes, workgroups -, the solver tail, ``launches_per_step``, the side streams,
the mode flags, and the sha256 of the result of a seeded run.  The inference kernels use no atomics and a fixed accumulation order, so the hashes
reproduce exactly: a mismatch is a behaviour change, not noise.  A launch-list mismatch is reported apart from a hash mismatch."""
import json
import os

import pytest
import torch

from tools import plan_signatures as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "plan_signatures.json")) as f:
        return ps.unpack(json.load(f))


@pytest.fixture(scope="module")
def tiny_hip_unet():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return ps.tiny_unet()


def test_the_golden_file_has_every_case(golden):
    assert sorted(golden) == sorted(ps.CASES)


@pytest.mark.parametrize("name", list(ps.CASES))
def test_plan_signature(name, golden, request):
    unet = request.getfixturevalue("tiny_hip_unet" if ps.CASES[name]["unet"] == "tiny" else "full_hip_unet")
    got, want = ps.run_case(name, unet), golden[name]
    assert len(got["engines"]) == len(want["engines"]), f"{name}: {len(got['engines'])} plans, recorded {len(want['engines'])}"
    for i, (g, w) in enumerate(zip(got["engines"], want["engines"])):
        for k in w:
            if g[k] != w[k]:
                n = None if g[k] is None or w[k] is None else next((j for j, (a, b) in enumerate(zip(g[k], w[k])) if a != b), min(len(g[k]), len(w[k])))
                pytest.fail(f"{name}: launch list of engine {i} {k} differs from launch {n} on: {len(g[k] or [])} launches, recorded {len(w[k] or [])}; "
                            f"there {g[k][n:n + 1] if n is not None else g[k]}, recorded {w[k][n:n + 1] if n is not None else w[k]}")
    for k in ("tail", "launches_per_step", "sides", "flags"):
        assert got[k] == want[k], f"{name}: {k} is {got[k]}, recorded {want[k]}"
    assert got["sha256"] == want["sha256"], f"{name}: same launch lists, other bits: the result's sha256 differs from the recorded one"
