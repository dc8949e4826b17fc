"""The argument checks of the pass-kernel entry points (runs without a GPU): every call of tests/golden/entry_refusals.json --
recorded by tests/entry_refusals.py from the library of the revision before the entry points shared one dtype dispatch, grid rule
and launch call -- returns the recorded code, PMOE_ERR_ARG, from this tree's library, and the argument list each was derived
from is still accepted."""
import json
from pathlib import Path

import pytest
import torch

from tests import entry_refusals

GOLDEN = Path(__file__).resolve().parent / "golden" / "entry_refusals.json"


# (with a GPU, a check that got lost would launch a kernel on the made-up pointers of the fixture)
@pytest.mark.skipif(torch.cuda.is_available(), reason="a lost check would launch on made-up device pointers")
def test_entry_points_return_the_recorded_refusals(monkeypatch):
    from pmoe_amd import hip
    for name in ("PMOE_STEM_WALK", "PMOE_STEM_WALK_KO"):          # the walk kernels' workgroup-count check: the default path
        monkeypatch.delenv(name, raising=False)
    lib = hip.load()
    table = json.loads(GOLDEN.read_text())
    # the fixture is the helper's table: a refusal added to one of them is recorded into the other
    assert [r[:2] for r in table] == json.loads(json.dumps(entry_refusals.rows()))
    assert len(table) > 400 and {r[2] for r in table} == {hip.ERR_ARG}
    got = [[name, args, entry_refusals.call(lib, name, args)] for name, args in (r[:2] for r in table)]
    assert [r for r, want in zip(got, table) if r != want] == []
    # no check got stricter either: every accepted argument list still passes all of them (without a GPU the launch behind them
    # fails in the runtime with a HIP error code > 0; pmoe_seg_loss_rows / _cp return their count)
    assert [name for name, (good, _) in entry_refusals.CASES.items() if entry_refusals.call(lib, name, good) <= 0] == []
