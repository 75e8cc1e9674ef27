"""The statuses of lsqr_set_option through the C ABI: every option whose rule can refuse a value (csrc/options.h: the
ranges, the one-of sets, the removed option) takes one value at its bound and refuses the one next to it with
LSQR_ERR_INVALID and a message that names it; an unknown name is LSQR_ERR_INVALID; batch_lanes is refused with
LSQR_ERR_STATE while a batch of the context or of one of its lanes is in flight.  The rules themselves, value by value,
are in tests/test_options.py (no GPU)."""
import pytest

from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context

pytestmark = pytest.mark.gpu

# option -> (accepted, refused, default)
VALIDATED = {
    "scan_index": (2, 3, 1), "scan_cpt": (1, 2, 0), "scan_pack": (0, 2, 1), "scan_recheck": (0, -1, 1),
    "scan_slab": (0, 2, 1), "scan_slab_gate": (8, 9, 3), "scan_hsplit": (128, 129, 0), "scan_kd_levels": (12, 13, 7),
    "lm_persist": (3, 4, 1), "lm_persist_wgs": (1024, 1025, 0), "lm_persist_timeout_ms": (60000, 60001, 2000),
    "many_round_hypotheses": (0, -1, 0), "scan_kd_after": (0, -1, 16384),
    "scan_ppl": (16, 3, 0), "scan_bound_merge": (8, 3, 0), "scan_block": (257, 255, 0), "scan_cell": (512, 128, 0),
    "scan_pairs_mfma": (0, 1, 0),
    "batch_lanes": (1, 5, 4),
}


def _status(ctx, name, value):
    try:
        ctx.set_option(name, value)
    except L.LsqrError as e:
        return e.status, str(e)
    return L.OK, ""


def test_statuses_of_set_option():
    data = synth.plane(2_000, 0.5, seed=5)[0]
    with Context(0) as ctx:
        ctx.set_model(L.PLANE, 3, 0.5)
        for name, (good, bad, default) in VALIDATED.items():
            assert _status(ctx, name, good)[0] == L.OK, name
            st, msg = _status(ctx, name, bad)
            assert st == L.ERR_INVALID and name in msg, (name, st, msg)   # (a refusal says which option refused)
            assert _status(ctx, name, default)[0] == L.OK, name           # back to the default
        assert _status(ctx, "batch_lanes", 0)[0] == L.ERR_INVALID
        assert _status(ctx, "scan_slab_gate", 0)[0] == L.ERR_INVALID
        assert _status(ctx, "lm_persist_timeout_ms", 0)[0] == L.ERR_INVALID
        st, msg = _status(ctx, "no_such_option", 1)
        assert st == L.ERR_INVALID and "unknown option no_such_option" in msg, (st, msg)
        assert _status(ctx, "", 1)[0] == L.ERR_INVALID

        # batch_lanes while batches are in flight: slot 0 is the context's own, slot 1 lane 1's (four lanes)
        ctx.upload(data)
        ctx.batch_fit_enqueue(3, 0, 64, slot=0)
        ctx.batch_fit_enqueue(3, 64, 64, slot=1)
        assert _status(ctx, "batch_lanes", 2)[0] == L.ERR_STATE
        assert _status(ctx, "batch_lanes", 5)[0] == L.ERR_INVALID        # the range comes first
        ctx.batch_fit_wait(0)
        assert _status(ctx, "batch_lanes", 2)[0] == L.ERR_STATE          # the lane's batch is still unread
        ctx.batch_fit_wait(1)
        assert _status(ctx, "batch_lanes", 2)[0] == L.OK
        assert _status(ctx, "batch_lanes", 4)[0] == L.OK
