"""The op-level entries' workspace on the device: a workspace of exactly the size the query names is enough and is not overrun, and -- where the
query is one walk that takes something -- a workspace one 256-byte unit below it is refused on the host with RU_ENOMEM.  The cases and the guarded
allocation are tests/op_cases.py's; every case is a few launches at a shape of a few thousand voxels (the two that need a full grid: ~10^5)."""
import pytest
import torch

from op_cases import GuardedWorkspace, cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    return cases()


def _bits(t):
    return t.contiguous().view(torch.uint8)


def test_query_sized_workspace_gives_the_same_bytes_and_is_not_overrun(table, monkeypatch):
    """(a) ws_bytes = the query: bit-equal to the same call with twice the workspace, the 4096 guard bytes behind ws_bytes untouched"""
    from brats2019_amd import _lib as L
    bad = []
    for name, _, run in table:
        twice, exact = GuardedWorkspace(lambda nbytes: 2 * nbytes), GuardedWorkspace()
        monkeypatch.setattr(L, "workspace", twice)
        ref = run()
        monkeypatch.setattr(L, "workspace", exact)
        got = run()
        same = len(ref) == len(got) > 0 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ref, got))
        finite = all(bool(torch.isfinite(t).all()) for t in got)
        if not (same and finite and twice.intact() and exact.intact()):
            bad.append((name, same, finite, twice.intact(), exact.intact()))
    assert not bad, bad


def test_workspace_one_unit_short_is_refused_on_the_host(table, monkeypatch):
    """(b) ws_bytes = query - 4096 - 256: RU_ENOMEM with "workspace too small", and what was enqueued before the refusal stayed inside ws_bytes"""
    from brats2019_amd import _lib as L
    bad, seen = [], 0
    for name, short, run in table:
        if not short:
            continue
        seen += 1
        ws = GuardedWorkspace(lambda nbytes: nbytes - 4096 - 256)
        monkeypatch.setattr(L, "workspace", ws)
        try:
            run()
            bad.append((name, "accepted"))
        except RuntimeError as e:
            if "(-2)" not in str(e) or "workspace too small" not in str(e):
                bad.append((name, str(e)))
        if not ws.intact():
            bad.append((name, "guard overwritten"))
    assert seen >= 20 and not bad, bad
