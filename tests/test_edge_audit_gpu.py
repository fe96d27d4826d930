"""Every case of the edge-case catalogue (``oracle.edge_cases``) through ``oracle.plan_audit.Auditor``: each kernel ``pv_gemm_conv`` / ``pv_attention`` can
dispatch to, and every other inference launcher, at its smallest ragged shape, with all the Auditor's checks unchanged - fp64 reference from the
launch's own parameter block, ``oracle.abi_ref``'s derived element and aggregate bounds (no tolerance of this file's own), outputs poisoned with NaN,
every byte of the output storages outside the described extents, a bit-identical second run - on guarded tensors: outputs sit inside a patterned arena a
stray tile cannot leave, inputs inside NaN, so a read outside an input's extent that reaches a result fails the finite check.

Since the newer loop features and the pre-loop conditioning joined the catalogue (the guided / stochastic / PAG steps, FreeU, the resize, the fp32 pointwise
launchers, ``pv_rows_mean``, the casts, patchify, the two embeds, ``pv_fusion_draw``; 51 cases, 345 launches, a group of them at the product's shapes) a case
may also name pairs of outputs that must agree bit for bit (the launchers' documented substitutions).

The 24 ``train-`` cases (180 launches) are single launches of 25 launchers of the training tape - the pointwise fp16 passes and their backwards, dropout, the
layout and exact-select launchers, the fixed-order reductions, the pieces of the identity loss, ``pv_layernorm_backward``, ``pv_wgrad_tn`` with its slab sum -
through the same ``test_edge_case`` with no tolerance of their own; no training plan is replayed.

Wall time of this file alone on one MI355X: 8.80 s for its 202 tests (7.1 s of it in the audits, 702 launches; the 24 training cases together
1.8 s, each below 0.2 s: none is among the file's eight slowest tests); the parent commit's file on the same box, same visit: 6.99 s for 178 tests
(522 launches); the whole GPU suite then: 234.04 s for 597 tests (EXPERIMENTS.md, "Training edge audit")."""
import time

import pytest
import torch

from oracle import edge_cases as E
from oracle.plan_audit import AuditError, Auditor

pytestmark = pytest.mark.gpu

T0 = time.time()


@pytest.fixture(scope="module")
def auditor():
    from photoverse_amd import _lib
    aud = Auditor(_lib.load())
    yield aud
    print("\nedge audit coverage (worst element error / bound, worst rel-L2 / aggregate bound):\n" + aud.table())
    print(f"edge audit: {aud.audited} launches of {len(E.CASES)} cases in {time.time() - T0:.1f} s")


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_edge_case(name, auditor):
    c = E.by_name(name)
    try:
        with E.environment(c.env):              # the per-call switches hold while the case is recorded and while its launches run
            rec = E.build(c, "cuda")
            assert not E.unguarded(rec)
            tags = [t[0] for t in rec.tags]
            for want in c.expect:
                assert want in tags, (want, tags)
            n = auditor.audit(name, rec)
            for a, b in getattr(rec, "same_bits", ()):      # pairs of outputs the case promises to be the same launch: bit for bit, not within a bound
                assert torch.equal(a, b), f"{name}: two launches that must be the same kernel on the same inputs differ in {(a != b).sum().item()} elements"
    except AssertionError:
        raise
    except Exception as e:                      # a HIP error: nothing more is started on a device that has faulted
        pytest.exit(f"{name}: {type(e).__name__}: {e}", returncode=3)
    assert n == len(rec.calls) and n > 0
    del rec
    torch.cuda.empty_cache()


def test_every_dispatchable_kernel_was_audited(auditor):
    """The kernel symbols audited above are exactly the ones the dispatch sweep of tests/test_edge_audit_cpu.py requires."""
    audited = {k[2] for k in auditor.rows if k[2].startswith(E.DISPATCHED)}
    required = set(E.swept_symbols()) - set(E.EXEMPT)
    assert audited == required, (sorted(required - audited), sorted(audited - required))
