"""CPU: a control for the shared comparison of tests/streamrig.py (call_streams, check_meters), which every
per-stream GPU file relies on.  A StreamRig runs on the FakeContext of tests/test_stream_random_host.py, which
answers every call from oracle streams of its own, so the clean run passes; then one deviation at a time is
planted in what the context hands back, and the shared code has to name the stream and the kind of difference.

Three streams -- I16 stereo, I24 mono, F32 stereo, rendered at 16, 24 and 16 bit, so rows of 4- and 6-byte frames
share the 6-byte pitch -- and calls of 64 and 7 frames with one pad byte per row."""
import ctypes as C
import types

import numpy as np
import pytest

from in_cwave_amd import abi, graph
from tests import streamrig as R
from tests.test_stream_random_host import FakeContext, _FakeLib

FS = 48000
INPUTS = [(FS, abi.FMT_I16, 2), (FS, abi.FMT_I24, 1), (FS, abi.FMT_F32, 2)]
RENDERS = [R.entry(), R.entry(b24=True), R.entry()]
CALLS = (64, 7)
LAST = 2                                # the last stream: 4-byte frames in a 6-byte-pitch row


def poke(addr, value=None, flip=0):
    b = (C.c_uint8 * 1).from_address(addr)
    b[0] = (b[0] ^ flip) if value is None else value


# what a plant does to a call's buffers: (out, out_stride, dbg, n) -> True once it has changed something
def pre_low_bit(out, stride, dbg, n):
    poke(dbg + (LAST * n + n // 2) * 16, flip=1)            # little endian: the lowest mantissa bit
    return True


def pre_minus_zero(out, stride, dbg, n):
    pre = np.frombuffer((C.c_uint64 * (3 * n * 2)).from_address(dbg), np.uint64)
    zeros = np.flatnonzero(pre == 0)
    if zeros.size:
        poke(dbg + int(zeros[0]) * 8 + 7, 0x80)
    return bool(zeros.size)


def last_rendered_byte(out, stride, dbg, n):
    poke(out + LAST * stride + n * 4 - 1, flip=0x10)
    return True


def byte_past_the_frames(out, stride, dbg, n):
    poke(out + 0 * stride + n * 4, 0)                       # stream 0: 4-byte frames, the row holds n * 6 + 1
    return True


def pad_byte_of_the_last_row(out, stride, dbg, n):
    poke(out + LAST * stride + stride - 1, 0)
    return True


def rows_swapped(out, stride, dbg, n):
    rows = np.frombuffer((C.c_uint8 * (3 * stride)).from_address(out), np.uint8).reshape(3, stride)
    rows[[0, LAST]] = rows[[LAST, 0]]
    return True


CALL_PLANTS = {
    "pre low bit": (pre_low_bit, 1, f"stream {LAST} ", "pre-render doubles differ"),
    "pre +0.0 to -0.0": (pre_minus_zero, 0, "stream 0 ", "pre-render doubles differ"),
    "last rendered byte": (last_rendered_byte, 1, f"stream {LAST} ", "rendered bytes differ"),
    "byte past the frames": (byte_past_the_frames, 0, "stream 0 ", "bytes written past its 256 bytes of frames"),
    "pad byte": (pad_byte_of_the_last_row, 1, f"stream {LAST} ", "bytes written past its 28 bytes of frames"),
    "rows swapped": (rows_swapped, 0, "stream 0 ", "rendered bytes differ"),
}
METER_PLANTS = {
    "clips": ("clips", "clips"),
    "peak ulp": ("peak_db", "peaks"),
    "desubnorm": ("desubnorm", "de-subnorm count"),
    "n_frame": ("n_frame", "n_frame"),
}


class PlantLib(_FakeLib):
    def icw_process_streams(self, h, first, count, inp, in_stride, out, out_stride, n, flags, dbg, hip_stream):
        rc = super().icw_process_streams(h, first, count, inp, in_stride, out, out_stride, n, flags, dbg, hip_stream)
        f = self.f
        if f.plant in CALL_PLANTS and f.calls == CALL_PLANTS[f.plant][1]:
            f.planted += CALL_PLANTS[f.plant][0](out, out_stride, dbg, n)
        f.calls += 1
        return rc


class PlantContext(FakeContext):
    """FakeContext with one deviation in what it hands back: in a call's buffers (CALL_PLANTS, in the call of
    that index) or in stream LAST's meters (METER_PLANTS)"""

    def __init__(self, plan, oracle, plant):
        super().__init__(plan, oracle)
        self.plant, self.calls, self.planted = plant, 0, 0
        self._lib = PlantLib(self)

    def meters(self, s):
        m = dict(super().meters(s))
        field = METER_PLANTS.get(self.plant, (None,))[0]
        if s == LAST and field == "clips":
            m["clips"] = (m["clips"][0], m["clips"][1] + 1)
        if s == LAST and field == "peak_db":
            m["peak_db"] = (float(np.nextafter(m["peak_db"][0], np.inf)), m["peak_db"][1])
        if s == LAST and field == "desubnorm":
            m["desubnorm"] += 1
        return m

    def n_frame(self, s):
        return super().n_frame(s) + (s == LAST and self.plant == "n_frame")


def run(oracle, plant=None):
    cfg = graph.default_config(FS)
    nodes = graph.graph_shift_master()
    plan = R.Plan(seed=0, S=3, env={}, cwave=False, frmod_scaled=cfg.frmod_scaled, inp=INPUTS[0], lst=(0, 0), rnd=R.RENDER_POOL[0],
                  hil=(cfg.hilbert_type, cfg.iir_kahan, cfg.iir_subnorm_reject), pool=[nodes], silent=frozenset(), ops=[])
    fake = types.SimpleNamespace(Context=lambda cfg, nodes, S: PlantContext(plan, oracle, plant))
    rig = R.StreamRig(fake, oracle, plan.config(), sum(CALLS), nodes=nodes, inputs=INPUTS, renders=RENDERS, pad=1)
    rig.raw[0] = rig.raw[0].copy()
    rig.raw[0][:8 * rig.fsz(0)] = 0                         # digital silence at the start: +0.0 pre-render doubles
    assert rig.osz == [4, 6, 4]
    for k, n in enumerate(CALLS):
        out = rig.step(n, device=bool(k), what="control")   # the device-pointer branch too (host arrays here)
        assert out.shape == (3, n * 6 + 1)
    rig.check("control")
    return rig.ctx


def test_clean_run_passes(oracle):
    ctx = run(oracle)
    assert ctx.calls == len(CALLS) and ctx.planted == 0


@pytest.mark.parametrize("plant", list(CALL_PLANTS) + list(METER_PLANTS))
def test_planted_deviation_is_caught(oracle, plant):
    with pytest.raises(AssertionError) as e:
        run(oracle, plant)
    stream, kind = CALL_PLANTS[plant][2:] if plant in CALL_PLANTS else (f"stream {LAST}", METER_PLANTS[plant][1])
    msg = str(e.value)
    assert msg.startswith("control stream") and stream in msg and kind in msg, msg
