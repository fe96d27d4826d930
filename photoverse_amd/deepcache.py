"""DeepCache-style feature reuse across denoising steps ([EXT] Ma, Fang, Wang, CVPR 2024): the host-side plan layer.

The deep, low-resolution part of the UNet changes slowly from step to step, so only every ``cache_interval``-th step would run the whole forward; the
steps between recompute the outermost down and up layers on the activation the last full step left in front of the matching up-path resnet.  This
module holds what that needs on the host and nothing that touches the device: which stages of ``unet.unet_stages`` a cached forward records
(``shallow_ranges``), where its cache point lies (``cache_entry``), the stacked time projection of just those resnets (``shallow_time_projection``), the
choice between a full and a cached step (``cached_step_is_full``) and the keyword checks.  No launch plan, loop or public keyword uses it yet
(sections 5 and 7): the fp32 reference of the definition lives in ``tests/test_deepcache_cpu.py``.

Definition.  ``p_1, p_2, ...`` are the skip-pushing stages (``skip > 0``) in order, ``p_1`` = ``conv_in``.  For a depth ``d`` the DOWN RANGE is
``stages[0 ... index(p_d)]`` (it pushes exactly ``d`` skips), the UP RANGE starts at the up-path resnet (``skip < 0``) in front of which the skip stack of
a full forward holds ``d`` entries - it pops ``p_d`` - and runs through ``conv_out``, and the CACHE POINT ``C_d`` is the activation that enters that resnet
in a full forward, before the never-materialised concat with the skip, with its column statistics.  Valid depths are 1 ... the number of skip-pushing
stages of the first resolution level, its downsample excluded (3 on SD-1.5), so a cached forward never leaves that level."""
from __future__ import annotations

import itertools
import numbers
from typing import Dict, Optional, Tuple

import torch

from .unet import time_projection


def max_cache_depth(stages) -> int:
    """The deepest valid ``cache_depth``: the skip-pushing stages of the first resolution level, its downsample excluded (3 on SD-1.5: ``conv_in`` and the
    two transformers of ``down_blocks.0``)."""
    return sum(1 for st in stages if st.skip > 0 and st.block == ("down", 0) and st.kind != "downsample")


def check_cache_depth(stages, depth) -> int:
    """``depth`` as an int in 1 ... ``max_cache_depth(stages)``; else a ``ValueError``."""
    top = max_cache_depth(stages)
    if not (isinstance(depth, numbers.Integral) and not isinstance(depth, bool) and 1 <= int(depth) <= top):
        raise ValueError(f"cache_depth must be an int in 1 ... {top} for this UNet (the skip-pushing stages of its first resolution level), got {depth!r}")
    return int(depth)


def check_cache_interval(interval, what: str = "cache_interval") -> Optional[int]:
    """``cache_interval`` as None (off: None or 1) or an int >= 2; anything else is a ``ValueError`` naming ``what``."""
    if interval is None:
        return None
    if not (isinstance(interval, numbers.Integral) and not isinstance(interval, bool) and interval >= 1):
        raise ValueError(f"{what} must be None or an int >= 1, got {interval!r}")
    return None if int(interval) == 1 else int(interval)


def cache_entry(stages, depth: int) -> int:
    """Index of the up-path resnet a cached forward of ``depth`` resumes at: the one in front of which the skip stack of a full forward holds ``depth``
    entries.  The activation entering it is the cache point ``C_depth``."""
    held = 0
    for i, st in enumerate(stages):
        if st.skip < 0:
            if held == depth:
                return i
            held -= 1
        elif st.skip > 0:
            held += 1
    raise ValueError(f"no up-path resnet of this walk pops skip {depth}")


def shallow_ranges(stages, depth) -> Tuple[tuple, tuple]:
    """The two ranges ``(first, last, adopts, writes)`` of a cached forward, in ``unet.plan_ranges``' form (indices into ``stages``, ``last`` inclusive): the
    down range from the latents, and the up range, which adopts ``"cache"`` - the cache point of the last full forward of the same branch."""
    d = check_cache_depth(stages, depth)
    push = [i for i, st in enumerate(stages) if st.skip > 0]
    return (0, push[d - 1], None, None), (cache_entry(stages, d), len(stages) - 1, "cache", None)


def shallow_time_projection(stages, depth) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, int]]:
    """``unet.time_projection`` restricted to the resnets a cached forward of ``depth`` records -> (fp16 weight, fp32 bias, resnet name -> first column):
    every ``time_emb_proj`` of the two ranges in recording order, its columns counted anew, zero rows up to whole 160-column tiles."""
    (a0, a1, _, _), (b0, b1, _, _) = shallow_ranges(stages, depth)
    own = [st for st in stages[a0:a1 + 1] + stages[b0:b1 + 1] if st.kind == "resnet"]
    wt, bt = time_projection(own)
    return wt, bt, dict(zip((st.name for st in own), itertools.accumulate([0] + [st.tcols for st in own])))


def cached_step_is_full(step: int, start: int, interval: Optional[int], valid: bool) -> bool:
    """The kind of step at table row ``step`` of a run started at row ``start``: a full one - every stage, the cache points rewritten - when caching is
    off (``interval`` None), when no full step has run since the loop was reset or given new conditioning (``valid`` False), or on every ``interval``-th
    row counted from ``start``; a cached one otherwise.  The solver tail, the step counter and the multistep history are the same in both."""
    return interval is None or not valid or (step - start) % interval == 0
