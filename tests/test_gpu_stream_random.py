"""GPU: random edit sequences over the four per-stream tables of one context at once -- DSP lists, inputs (real
and CWAVE), renders and Hilbert converters, the context-wide setters, track opens, subset and one-stream calls,
host and device pointers, under the ICW_K1_MODE / ICW_RENDER / ICW_BLOCK switches -- against one oracle.Stream
per stream (tests/streamrig.py: plan, model and rig; tests/test_stream_random_host.py checks those without a
device, and that the plans cover what this file is for).  After every edit the four counts and every stream's
render size; after every call, for every stream of the call, bit for bit: the pre-render doubles (when asked
for), the rendered bytes at the stream's own frame size, the guard bytes past them, clips, peak dB bits,
de-subnorm counts and the frame counter.  Nothing here has a tolerance.

ICW_STREAM_SEEDS=<n> runs more seeds (a multiple of BATCH); a failure names its seed, switches and ops."""
import os

import pytest

from in_cwave_amd import abi
from tests import streamrig as R

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("ICW_STREAM_SEEDS", 64))      # the range the CPU coverage test surveys
BATCH = 8

_K1 = {}
_RAN = []


def after_call(rig, op):
    """the K1 form of a Hilbert-mixed real-input call: the forced one where it exists (the row form has no
    baseline summation: entries that are not all Kahan + reject run the lane form), either in automatic mode"""
    tab, first, count = rig.tab, op.a["first"], op.a["count"]
    if R.is_cw(tab.inp[first]) or tab.count("hilbert", first, count) < 2:
        return
    k1 = rig.ctx.last_k1_kernel()
    kr = all(h[1] and h[2] for h in tab.hil[first:first + count])
    mode = rig.plan.env.get("ICW_K1_MODE")
    assert k1 in (abi.K1_ROW, abi.K1_LANE), rig.where(op)
    if mode == "plain" or not kr:
        assert k1 == abi.K1_LANE, f"{rig.where(op)}: K1 form {k1}"
    elif mode == "row":
        assert k1 == abi.K1_ROW, f"{rig.where(op)}: K1 form {k1}"
    _K1[k1] = _K1.get(k1, 0) + 1


def run_seed(icw, oracle, monkeypatch, seed):
    plan = R.make_plan(seed)
    for name in R.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in plan.env.items():
        monkeypatch.setenv(name, v)                      # read at icw_create
    ctx = icw.Context(plan.config(), plan.nodes(), plan.S)
    try:
        R.Rig(plan, ctx, oracle, after_call).run()
    finally:
        ctx.close()


@pytest.mark.parametrize("batch", range(SEEDS // BATCH))
def test_random_edit_sequences(icw, oracle, monkeypatch, batch):
    for seed in range(batch * BATCH, (batch + 1) * BATCH):
        run_seed(icw, oracle, monkeypatch, seed)
    _RAN.append(batch)


def test_both_k1_forms_ran_hilbert_mixed_calls():
    """(runs after the batches)"""
    if not _RAN:
        pytest.skip("batches not run in this session")
    assert _K1.get(abi.K1_ROW, 0) > 0 and _K1.get(abi.K1_LANE, 0) > 0, _K1
