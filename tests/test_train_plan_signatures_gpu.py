"""The training plans against the signatures recorded at the commit ``tests/golden/train_plan_signatures.json`` names
(``tools/plan_signatures.py --train``): every recorder of a ``TrainStep`` launch for launch - the main tape's forward and backward plan and, with the
face loss, the conditioning, stacking, loop, last-step and backward recorders of that branch -, ``dropout_sites``, ``fusion_names``, and the sha256 of
(loss, face loss, every trainable gradient) after the first, eager step and after the second, replayed one on the same seeded inputs.  The training
kernels use no atomics and a fixed accumulation order, so the hashes reproduce exactly.  Without LoRA dropout the two steps are the same computation
and their hashes agree (``test_training_step_is_bit_reproducible``); with it the masks are keyed on a device-side counter every forward advances, so
the replayed step draws other masks than the eager one and each of the two hashes is pinned on its own."""
import json
import os

import pytest

from tools import plan_signatures as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "train_plan_signatures.json")) as f:
        return ps.unpack_train(json.load(f))


def test_the_golden_file_has_every_training_case(golden):
    assert sorted(golden) == sorted(ps.TRAIN_CASES)


@pytest.mark.parametrize("name", list(ps.TRAIN_CASES))
def test_train_plan_signature(name, golden, request):
    c = ps.TRAIN_CASES[name]
    got, want = ps.run_train_case(name, request.getfixturevalue("full_hip_unet") if c["unet"] == "full" else None), golden[name]
    assert sorted(got["recorders"]) == sorted(want["recorders"])
    for k, w in want["recorders"].items():
        g = got["recorders"][k]
        if g != w:
            n = next((j for j, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            pytest.fail(f"{name}: launch list of {k} differs from launch {n} on: {len(g)} launches, recorded {len(w)}; there {g[n:n + 1]}, "
                        f"recorded {w[n:n + 1]}")
    for k in ("dropout_sites", "fusion_names"):
        assert got[k] == want[k], f"{name}: {k} is {got[k]}, recorded {want[k]}"
    assert len(got["sha256"]) == len(want["sha256"]) == (2 if c["run"] else 0)
    if c["run"] and not c["lora_dropout"]:
        assert got["sha256"][0] == got["sha256"][1], f"{name}: the replayed step's bits differ from the eager step's"
    assert got["sha256"] == want["sha256"], f"{name}: same launch lists, other bits: the sha256 of loss and gradients differs from the recorded one"
