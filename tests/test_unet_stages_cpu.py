"""``unet_stages``: the one walk of a UNet forward both the inference plans and the training tape record, and ``plan_ranges``: the plan kinds of
``UNetEngine`` as ranges of it.  Host-side: the tiny UNet on the CPU, the SD-v1.5-sized one on ``meta``."""
from collections import Counter

import pytest
import torch

from oracle.unet_ref import TINY_CONFIG
from photoverse_amd.unet import (ResnetBlock2D, UNet2DConditionModel, plan_ranges, time_projection, time_projection_width, transformer_names,
                                 unet_stages)

TINY_TRANSFORMERS = ("down_blocks.0.attentions.0", "mid_block.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1")
#: per UNet: resnets, transformers, downsamples, upsamples, stacked width
SIZES = {"tiny": (8, 4, 1, 1, 4160), "sd15": (22, 16, 3, 3, 20160)}


@pytest.fixture(scope="module", params=["tiny", "sd15"])
def case(request):
    if request.param == "tiny":
        unet = UNet2DConditionModel(**TINY_CONFIG)
    else:
        with torch.device("meta"):
            unet = UNet2DConditionModel()
    return request.param, unet, unet_stages(unet)


def test_counts_per_kind_and_stacked_width(case):
    name, unet, stages = case
    n = Counter(st.kind for st in stages)
    assert (n["resnet"], n["transformer"], n["downsample"], n["upsample"], time_projection_width(stages)) == SIZES[name]
    assert n["conv_in"] == n["conv_out"] == 1 and stages[0].kind == "conv_in" and stages[-1].kind == "conv_out" and len(stages) == sum(n.values())
    assert isinstance(stages, tuple) and all(isinstance(st, tuple) for st in stages)
    assert all(unet.get_submodule(st.name) is st.module for st in stages)


def test_transformer_names_are_the_pinned_ones(case):
    name, unet, stages = case
    names = tuple(st.name for st in stages if st.kind == "transformer")
    assert names == transformer_names(unet)
    if name == "tiny":
        assert names == TINY_TRANSFORMERS
    else:       # what tests/test_pag_cpu.py pins of the SD-v1.5 order
        assert names[:2] == ("down_blocks.0.attentions.0", "down_blocks.0.attentions.1") and names[6] == "mid_block.attentions.0" and len(names) == 16


def test_resnets_in_module_order_with_cumulative_offsets(case):
    _, unet, stages = case
    res = [st for st in stages if st.kind == "resnet"]
    mods = [m for m in unet.modules() if isinstance(m, ResnetBlock2D)]
    assert len(res) == len(mods) and all(st.module is m for st, m in zip(res, mods))
    off = 0
    for st, m in zip(res, mods):
        assert (st.toff, st.tcols) == (off, m.conv1.out_channels)
        off += m.conv1.out_channels
    assert off <= time_projection_width(stages) < off + 160 and time_projection_width(stages) % 160 == 0
    assert all((st.toff, st.tcols) == (0, 0) for st in stages if st.kind != "resnet")


def test_stacked_projection_rows_are_the_resnets_own():
    stages = unet_stages(UNet2DConditionModel(**TINY_CONFIG))
    wt, bt = time_projection(stages)
    assert wt.shape == (4160, 1280) and wt.dtype == torch.float16 and bt.shape == (4160,) and bt.dtype == torch.float32
    for st in stages:
        if st.kind == "resnet":
            lin = st.module.time_emb_proj
            assert torch.equal(wt[st.toff:st.toff + st.tcols], lin.weight.detach().half()) and torch.equal(bt[st.toff:st.toff + st.tcols], lin.bias.detach())
    used = sum(st.tcols for st in stages)
    assert not wt[used:].any() and not bt[used:].any()


def test_levels_change_by_one_at_the_samplers_only(case):
    _, _, stages = case
    assert stages[0].level == stages[-1].level == 0
    for a, b in zip(stages, stages[1:]):
        assert b.level - a.level == {"downsample": 1, "upsample": -1}.get(a.kind, 0)


def test_the_skip_stack_balances_and_feeds_the_up_path_norms(case):
    _, unet, stages = case
    ch, skips = None, []
    for st in stages:
        if st.kind == "resnet":
            if st.skip < 0:
                assert st.block[0] == "up" and st.module.norm1.num_channels == ch + skips.pop()
            else:
                assert st.module.norm1.num_channels == ch
            ch = st.module.conv1.out_channels
        elif st.kind == "conv_in":
            ch = st.module.out_channels
        elif st.kind == "conv_out":
            assert st.module.in_channels == ch
        assert st.skip in (-1, 0, 1) and (st.skip >= 0 or st.kind == "resnet")
        if st.skip > 0:
            skips.append(ch)
    assert not skips


def _sd15_stages():
    with torch.device("meta"):
        return unet_stages(UNet2DConditionModel())


def test_whole_and_prefix_ranges():
    stages = _sd15_stages()
    n = len(stages)
    assert plan_ranges(stages) == ((0, n - 1, None, None),)
    (first, last, adopts, writes), = plan_ranges(stages, "prefix")
    assert (first, last, adopts, writes) == (0, 2, None, "prefix_out")
    assert [st.kind for st in stages[first:last + 1]] == ["conv_in", "resnet", "transformer"]
    # a plan given the prefix adopts those three stages' tensors and resumes inside the third, the first transformer
    assert plan_ranges(stages, prefix=True) == ((2, n - 1, "prefix", None),)


def test_split_ranges_partition_the_walk():
    stages = _sd15_stages()
    n = len(stages)
    head, tail = plan_ranges(stages, "outer", 2)
    mid, = plan_ranges(stages, "mid", 2)
    assert (head[0], tail[1]) == (0, n - 1) and mid[0] == head[1] + 1 and tail[0] == mid[1] + 1       # head | mid | tail is the whole list
    assert stages[head[1]].kind == "downsample" and stages[head[1]].block == ("down", 1) and stages[mid[1]].kind == "upsample"
    assert stages[mid[1]].block == ("up", 1) and stages[mid[0]].level == 2 and stages[tail[0]].level == 1
    assert (head[2], head[3]) == (None, "mid_in") and (mid[2], mid[3]) == ("mid_in", "mid_out") and (tail[2], tail[3]) == ("mid_out", None)
    # skips never cross the seams the wrong way: the head leaves exactly what the tail pops
    assert sum(st.skip for st in stages[:head[1]]) == -sum(st.skip for st in stages[tail[0]:])
    # with the shared prefix only the head's start moves
    assert plan_ranges(stages, "outer", 2, prefix=True) == ((2, head[1], "prefix", "mid_in"), tail)
    for split in (1, 3):
        h2, t2 = plan_ranges(stages, "outer", split)
        m2, = plan_ranges(stages, "mid", split)
        assert (h2[0], m2[0], t2[0], t2[1]) == (0, h2[1] + 1, m2[1] + 1, n - 1) and stages[m2[0]].level == split and stages[t2[0]].level == split - 1


@pytest.mark.parametrize("at", ["mid_block.attentions.0", "up_blocks.1.attentions.0"])
def test_trunk_range_starts_at_the_named_transformer(at):
    stages = _sd15_stages()
    (first, last, adopts, writes), = plan_ranges(stages, trunk_at=at, prefix=True)      # the trunk holds the prefix: prefix= changes nothing
    assert stages[first].name == at and stages[first].kind == "transformer" and (last, adopts, writes) == (len(stages) - 1, "trunk", None)
