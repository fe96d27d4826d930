"""The order of a denoising step.  ``tests/golden/step_traces.json`` holds what ``DenoiseLoop._step_eager()`` issued at the commit the file names, before
the step became data (``tools/plan_signatures.py --trace``): every recorder run and every stream wait with its streams, and how many streams a build and
a ``capture()`` construct.  The loops of the tree must issue exactly that, and their ``schedule`` must be what the engine lists say.  Only plans are
built: the recorders and the waits are logged, not run."""
import json
import os

import pytest
import torch

from tools import plan_signatures as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "step_traces.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def tiny_hip_unet():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return ps.tiny_unet()


def expected_schedule(loop):
    """The step written out from the engine lists: groups in sequence, lanes side by side, recorders of a lane in order."""
    groups = [((e.rec,),) for e in loop.engines_p]
    if loop.merge_lowres:
        (eu,), (ec,), (em,) = loop.engines_u, loop.engines_c, loop.engines_m
        groups += [((eu.rec_head,), (ec.rec_head,)), ((em.rec,),), ((eu.rec_tail,), (ec.rec_tail,))]
    else:
        follows = {id(c): p for c, p in zip(loop.engines_c, loop.engines_p_attn)}
        groups.append(tuple((e.rec, follows[id(e)].rec) if id(e) in follows else (e.rec,) for e in loop.engines_u + loop.engines_c + loop.engines_i))
    groups.append(((loop.tail,),))
    if not loop.two_streams:
        groups = [(tuple(rec for lane in lanes for rec in lane),) for lanes in groups]
    return tuple(groups)


def test_the_golden_file_has_every_loop(golden):
    assert sorted(golden) == sorted(ps.TRACE_CASES) == sorted(k for k, c in ps.CASES.items() if "kw" in c)


@pytest.mark.parametrize("name", list(ps.TRACE_CASES))
def test_step_trace_and_schedule(name, golden, request):
    unet = request.getfixturevalue("tiny_hip_unet" if ps.TRACE_CASES[name]["unet"] == "tiny" else "full_hip_unet")
    loop, got = ps.trace_case(name, unet)
    want = golden[name]
    print(f"{name}: {len(got['trace'])} entries, streams {got['streams_built']} + {got['streams_capture']}")
    assert got["streams_built"] == want["streams_built"] == len(loop._sides) and got["streams_capture"] == want["streams_capture"] == 1
    n = next((i for i, (a, b) in enumerate(zip(got["trace"], want["trace"])) if a != b), min(len(got["trace"]), len(want["trace"])))
    assert got["trace"] == want["trace"], f"{name}: the step differs from entry {n} on: {got['trace'][n:n + 1]}, recorded {want['trace'][n:n + 1]}"
    exp = expected_schedule(loop)
    assert isinstance(loop.schedule, tuple) and len(loop.schedule) == len(exp)
    for group, egroup in zip(loop.schedule, exp):
        assert isinstance(group, tuple) and len(group) == len(egroup) <= len(loop._sides) + 1
        for lane, elane in zip(group, egroup):
            assert isinstance(lane, tuple) and len(lane) == len(elane) and all(a is b for a, b in zip(lane, elane))
    # every recorder of a step runs exactly once (an outer plan's ``rec`` is a view of its head and tail for introspection: those two run)
    ran = [rec for group in loop.schedule for lane in group for rec in lane]
    owned = {id(loop.tail)} | {id(r) for e in loop.all_engines for r in ((e.rec,) if e.rec_head is None else (e.rec_head, e.rec_tail))}
    assert len({id(r) for r in ran}) == len(ran) and {id(r) for r in ran} == owned
