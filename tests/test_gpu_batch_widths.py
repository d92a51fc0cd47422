"""Ragged batch widths: every kernel that maps streams onto lanes, 16-lane rows, waves or workgroups, at
widths that leave a partial last group behind at least one full one -- and every stream checked.

The rest of the suite runs these kernels either at 1-9 streams (one partial wave: no index arithmetic
across groups) or at 256 / 2048 / 4096 (every wave and lane group full: no tail guard runs).  Here each
case runs S distinct generated inputs (synth.batch_pcm, no tiling) through two calls of ragged lengths --
the second one depends on what the advance kernels and the state hand-off left for every stream -- and
compares EVERY stream with its own oracle.Stream: the rendered bytes, the pre-render doubles bit for bit
(any NaN equals any NaN, as in test_gpu_graph_random.py), the meters (clips, peak_db, de-subnorm count),
the frame counter, and for FP_CHECK the census.  All S output rows must be pairwise distinct (the oracle's
rows are checked first: if those collide the inputs are at fault), and the K1 that ran is asserted.

oracle.process_streams runs fresh streams and drops them, so it cannot give the meters and counters
after the second call; the rig keeps one oracle.Stream per stream on synth.cpu_workers() threads instead.

The widths at which the host switches kernels by itself come from the device's CU count, with the
host's formulas restated below (CallPlan::pick_k1, CallPlan::k3_args): nothing here hard-codes 257 or
513.  test_rig_reports_swapped_and_duplicated_streams is the negative control, on the CPU.
"""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth

gpu = pytest.mark.gpu

FS = 48000
CALLS = (300, 277)            # ragged, and no multiple of any filter order or of the 20-sample render block

SWITCHES = ("ICW_K1_MODE", "ICW_RENDER", "ICW_DEDUP", "ICW_K1_WG", "ICW_K1_WPC", "ICW_BLOCK", "ICW_DITH_PAR",
            "ICW_STREAM1", "ICW_CU_SPLIT", "ICW_SERIALIZE", "ICW_FIRST_BLOCK", "ICW_TAPER", "ICW_SETS")


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    """a case runs under the switches it names and no others (icw_create reads them once per context)"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


# ---------------------------------------------------------------- the host's geometry, restated --
K1_WPC = 2                    # IcwTuning::k1_wpc, the default
ROW_RENDER_MAX = 2048         # kRowRenderMax (icw_ctx.h): channels up to which the render runs a row per channel


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def row_waves(S, dedup):
    """CallPlan::pick_k1: the row kernel holds four chain slots per wave and filter; 2 S slots, S under
    the mono dedup"""
    return ((S if dedup else 2 * S) + 3) // 4 * 2


def auto_k1(S, dedup, cus, row_ok=True):
    """CallPlan::pick_k1, no ICW_K1_MODE: the row kernel while its waves fit k1_wpc per CU on half the chip"""
    return abi.K1_ROW if row_ok and row_waves(S, dedup) <= (cus // 2) * K1_WPC else abi.K1_LANE


def first_plain_width(dedup, cus):
    """the first width past the row threshold whose last plain-K1 lane group (launch_k1_t: 32 streams, 64
    under the dedup) is partial"""
    S = 1
    while auto_k1(S, dedup, cus) == abi.K1_ROW:
        S += 1
    while S % (64 if dedup else 32) == 0:
        S += 1
    return S


def last_odd_row_width(cus):
    """the last odd stereo width the row kernel still takes by itself: 2 S slots, so half a wave at the end"""
    S = first_plain_width(False, cus)
    while S > 1 and (auto_k1(S, False, cus) != abi.K1_ROW or S % 2 == 0):
        S -= 1
    return S


def first_lane_render_width():
    """CallPlan::k3_args: a3.row while n_gen = 2 S <= kRowRenderMax; the first stereo width past it whose
    last lane-per-channel wave ((n_gen + 63) / 64 waves, icw_launch_render) is partial"""
    S = ROW_RENDER_MAX // 2 + 1
    while (2 * S) % 64 == 0:
        S += 1
    return S


def last_odd_row_render_width():
    """the last odd stereo width of the row render ((n_gen + 3) / 4 waves): half a wave at the end"""
    S = ROW_RENDER_MAX // 2
    return S if S % 2 else S - 1


# ---------------------------------------------------------------------------------- the rig ----
def differing(a, b):
    """indices where two double arrays differ bit for bit, any NaN equal to any NaN (the sign of a default
    NaN differs between x86 and the GPU; the render maps every NaN to the same integer)"""
    bad = a.view(np.uint64) != b.view(np.uint64)
    return np.flatnonzero(bad & ~(np.isnan(a) & np.isnan(b)))


def bundle(out, pre, meters, n_frame, census=None):
    """per-stream results of one side: out [S, bytes] uint8, pre [S, n, 2] float64 or None, and lists of
    S meters dicts, frame counters and (FP_CHECK) census arrays"""
    return {"out": out, "pre": pre, "meters": meters, "n_frame": n_frame, "census": census}


def stream_diffs(got, ref, ids=None):
    """[(stream, what differs)] over EVERY stream of ref; empty when the two sides agree"""
    S = len(ref["meters"])
    ids = list(range(S)) if ids is None else ids
    errs = []
    if len(got["meters"]) != S or got["out"].shape != ref["out"].shape:
        return [(-1, f"shapes differ: {got['out'].shape} against {ref['out'].shape}")]
    for i in range(S):
        why = []
        bad = np.flatnonzero(got["out"][i] != ref["out"][i])
        if bad.size:
            why.append(f"{bad.size} output bytes, first at {bad[:3].tolist()}")
        if ref["pre"] is not None:
            bad = differing(got["pre"][i].reshape(-1), ref["pre"][i].reshape(-1))
            if bad.size:
                why.append(f"{bad.size} pre-render doubles, first at {bad[:3].tolist()}")
        m, r = got["meters"][i], ref["meters"][i]
        if not (tuple(m["clips"]) == tuple(r["clips"]) and tuple(m["peak_db"]) == tuple(r["peak_db"])
                and m["desubnorm"] == r["desubnorm"]):
            why.append(f"meters {m} != {r}")
        if got["n_frame"][i] != ref["n_frame"][i]:
            why.append(f"n_frame {got['n_frame'][i]} != {ref['n_frame'][i]}")
        if ref["census"] is not None and not np.array_equal(got["census"][i], ref["census"][i]):
            why.append(f"census {got['census'][i].tolist()} != {ref['census'][i].tolist()}")
        if why:
            errs.append((ids[i], "; ".join(why)))
    return errs


def duplicate_rows(out):
    """groups of streams whose output rows are byte for byte the same (none: nothing cross-wired or doubled)"""
    seen = {}
    for s in range(out.shape[0]):
        seen.setdefault(out[s].tobytes(), []).append(s)
    return [g for g in seen.values() if len(g) > 1]


def assert_same(got, ref, label, ids=None):
    errs = stream_diffs(got, ref, ids)
    S = len(ref["meters"])
    assert not errs, (f"{label}: {len(errs)} of {S} streams differ, streams {[s for s, _ in errs][:8]}: "
                      f"{[f'stream {s}: {w}' for s, w in errs[:3]]}")


def assert_distinct(ref_out, got_out, label):
    dup = duplicate_rows(ref_out)
    assert not dup, f"{label}: the ORACLE's rows collide for streams {dup[:4]} -- change the inputs"
    dup = duplicate_rows(got_out)
    assert not dup, f"{label}: {len(dup)} groups of streams share an output row, first {dup[:4]}"


def oracle_run(oracle, cfg, nodes, raw, calls, census=False):
    """every row of raw through its own oracle.Stream, call by call"""
    S = raw.shape[0]
    fsz = abi.FMT_BYTES[cfg.in_format] * cfg.in_channels

    def one(s):
        st = oracle.Stream(cfg, nodes)
        outs, pres, t = [], [], 0
        for n in calls:
            o, p = st.process(raw[s, t * fsz:(t + n) * fsz], n, want_pre=True)
            outs.append(o)
            pres.append(p)
            t += n
        return (np.concatenate(outs), np.concatenate(pres), st.meters(), st.n_frame(),
                st.fp_census() if census else None)
    with ThreadPoolExecutor(synth.cpu_workers()) as pool:
        res = list(pool.map(one, range(S)))
    return bundle(np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), [r[2] for r in res],
                  [r[3] for r in res], [r[4] for r in res] if census else None)


def gpu_run(icw, cfg, nodes, raw, calls, k1, census=False):
    """the same rows through one context; the K1 of every call is asserted"""
    S = raw.shape[0]
    ctx = icw.Context(cfg, nodes, S)
    fsz = ctx.fsz
    outs, pres, t = [], [], 0
    for n in calls:
        o, p = ctx.process(np.ascontiguousarray(raw[:, t * fsz:(t + n) * fsz]), n, want_pre=True)
        assert ctx.last_k1_kernel() == k1, f"K1 kernel {ctx.last_k1_kernel()} ran, {k1} expected"
        outs.append(o)
        pres.append(p)
        t += n
    got = bundle(np.concatenate(outs, axis=1), np.concatenate(pres, axis=1), [ctx.meters(s) for s in range(S)],
                 [ctx.n_frame(s) for s in range(S)], [ctx.fp_census(s) for s in range(S)] if census else None)
    ctx.close()
    return got


def run_case(oracle, icw, label, cfg, nodes, S, k1, raw=None, census=False):
    t0 = time.perf_counter()
    if raw is None:
        raw = synth.batch_pcm(S, sum(CALLS), cfg.sample_rate, channels=cfg.in_channels, fmt=cfg.in_format,
                              workers=synth.cpu_workers())
    assert raw.shape[0] == S
    got = gpu_run(icw, cfg, nodes, raw, CALLS, k1, census)
    ref = oracle_run(oracle, cfg, nodes, raw, CALLS, census)
    print(f"[batch widths] {label}: S={S} in {time.perf_counter() - t0:.2f} s")
    assert_same(got, ref, label)
    assert_distinct(ref["out"], got["out"], label)


def shift_master():
    """Shift(in -> A, +2 / -2 Hz) + Master(A): the Shift makes the second call depend on every stream's frame
    counter; the Master's gain of 3.0 (default 0.8) drives most streams into clipping now and then, so the
    clip counters differ from stream to stream like the peaks do"""
    return [graph.master(inputs=("A",), gain=3.0), graph.shift(inputs=("in",), out="A")]


def stereo_cfg(htype=1):
    return graph.default_config(FS, hilbert_type=htype)


def mono_cfg():
    return graph.default_config(FS, channels=1)


def shaped_cfg():
    """24-bit TPDF + MEW44: a serial render"""
    cfg = graph.default_config(FS, need24bits=True)
    cfg.render.render_type, cfg.render.nshape_type = abi.RENDER_TPDF, abi.NSHAPE_MEW44
    return cfg


# ------------------------------------------------------------------------ the recurrence (K1) ----
@gpu
@pytest.mark.parametrize("S", [31, 33, 65])
def test_plain_k1_stereo(oracle, icw, monkeypatch, S):
    """launch_k1_t: 128-lane groups of 32 streams"""
    monkeypatch.setenv("ICW_K1_MODE", "plain")
    run_case(oracle, icw, f"plain K1 stereo {S}", stereo_cfg(), shift_master(), S, abi.K1_LANE)


@gpu
def test_plain_k1_stereo_automatic(oracle, icw):
    """the first stereo width the host gives to the plain kernel by itself (257 on 256 CUs)"""
    cus = n_cu()
    S = first_plain_width(False, cus)
    assert auto_k1(S - 1, False, cus) == abi.K1_ROW or (S - 1) % 32 == 0
    run_case(oracle, icw, f"plain K1 stereo automatic ({cus} CUs)", stereo_cfg(), shift_master(), S,
             abi.K1_LANE)


@gpu
@pytest.mark.parametrize("S", [63, 65, 129])
def test_plain_k1_mono_dedup(oracle, icw, monkeypatch, S):
    """launch_k1_t under the mono dedup: 64 streams per group, the right converters' state a copy"""
    monkeypatch.setenv("ICW_K1_MODE", "plain")
    run_case(oracle, icw, f"plain K1 mono dedup {S}", mono_cfg(), shift_master(), S, abi.K1_LANE)


@gpu
def test_plain_k1_mono_dedup_automatic(oracle, icw):
    """the first mono width past the row threshold (513 on 256 CUs)"""
    cus = n_cu()
    S = first_plain_width(True, cus)
    run_case(oracle, icw, f"plain K1 mono dedup automatic ({cus} CUs)", mono_cfg(), shift_master(), S,
             abi.K1_LANE)


@gpu
def test_plain_k1_mono_dedup_off(oracle, icw, monkeypatch):
    monkeypatch.setenv("ICW_K1_MODE", "plain")
    monkeypatch.setenv("ICW_DEDUP", "0")
    run_case(oracle, icw, "plain K1 mono, dedup off 33", mono_cfg(), shift_master(), 33, abi.K1_LANE)


@gpu
@pytest.mark.parametrize("S", [33, "last odd before the threshold"])
def test_row_k1_stereo(oracle, icw, monkeypatch, S):
    """launch_k1r_t: four chain slots per wave, 2 S slots; an odd S ends in half a wave (255 on 256 CUs)"""
    monkeypatch.setenv("ICW_K1_MODE", "row")
    if not isinstance(S, int):
        S = last_odd_row_width(n_cu())
        assert S % 2 == 1 and auto_k1(S, False, n_cu()) == abi.K1_ROW
    run_case(oracle, icw, f"row K1 stereo {S}", stereo_cfg(), shift_master(), S, abi.K1_ROW)


@gpu
@pytest.mark.parametrize("S", [65, 66, 67])
def test_row_k1_mono_dedup(oracle, icw, monkeypatch, S):
    """launch_k1r_t under the dedup: S slots, four per wave -- one, two and three live rows in the last"""
    monkeypatch.setenv("ICW_K1_MODE", "row")
    run_case(oracle, icw, f"row K1 mono dedup {S}", mono_cfg(), shift_master(), S, abi.K1_ROW)


@gpu
@pytest.mark.parametrize("wg", [1, 4])
def test_row_k1_workgroup_waves(oracle, icw, monkeypatch, wg):
    """ICW_K1_WG: 7 stereo streams are 14 slots, 8 waves -- whole one-wave or four-wave workgroups, the last
    wave half full"""
    monkeypatch.setenv("ICW_K1_MODE", "row")
    monkeypatch.setenv("ICW_K1_WG", str(wg))
    run_case(oracle, icw, f"row K1 {wg} waves per workgroup, 7", stereo_cfg(), shift_master(), 7,
             abi.K1_ROW)


@gpu
@pytest.mark.parametrize("htype", [0, 1, 2, 3, 4, 5])
def test_plain_k1_every_hilbert_type(oracle, icw, monkeypatch, htype):
    """orders 15, 18, 19 and 20 are separate instantiations of icw_iir_state"""
    monkeypatch.setenv("ICW_K1_MODE", "plain")
    run_case(oracle, icw, f"plain K1 Hilbert type {htype}, 33", stereo_cfg(htype), shift_master(), 33,
             abi.K1_LANE)


@gpu
def test_baseline_summation_falls_to_plain_k1(oracle, icw):
    """no Kahan, no reject: the row kernel does not serve it (pick_k1's row_ok), whatever the width"""
    cfg = stereo_cfg()
    cfg.iir_kahan, cfg.iir_subnorm_reject = 0, 0
    assert auto_k1(33, False, n_cu(), row_ok=False) == abi.K1_LANE
    run_case(oracle, icw, "baseline summation 33", cfg, shift_master(), 33, abi.K1_LANE)


# ------------------------------------------------------------------------- the serial renders ----
@gpu
@pytest.mark.parametrize("S", [31, 33])
def test_lane_render(oracle, icw, monkeypatch, S):
    """icw_launch_render, a lane per channel: (n_gen + 63) / 64 waves, 62 and 66 channels; two launch blocks"""
    monkeypatch.setenv("ICW_RENDER", "serial")
    monkeypatch.setenv("ICW_BLOCK", "256")
    run_case(oracle, icw, f"lane render {S}", shaped_cfg(), shift_master(), S,
             auto_k1(S, False, n_cu()))


@gpu
def test_lane_render_automatic(oracle, icw, monkeypatch):
    """the first width past kRowRenderMax channels: 1025 stereo streams, 33 waves, two live lanes in the last"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    S = first_lane_render_width()
    assert 2 * S > ROW_RENDER_MAX and (2 * S) % 64
    run_case(oracle, icw, f"lane render automatic {S}", shaped_cfg(), shift_master(), S,
             auto_k1(S, False, n_cu()))


@gpu
@pytest.mark.parametrize("S", [33, "last odd up to the threshold"])
def test_row_render(oracle, icw, monkeypatch, S):
    """icw_launch_render, a row per channel with a companion wave: (n_gen + 3) / 4 chain waves, an odd width
    leaves half of the last one (1023: the last odd width at or below kRowRenderMax channels)"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    if not isinstance(S, int):
        S = last_odd_row_render_width()
    assert 2 * S <= ROW_RENDER_MAX and S % 2 == 1
    run_case(oracle, icw, f"row render {S}", shaped_cfg(), shift_master(), S,
             auto_k1(S, False, n_cu()))


@gpu
@pytest.mark.parametrize("rtype,b24", [(abi.RENDER_GAUSS, True), (abi.RENDER_STPDF, False)])
def test_dithered_flat_render(oracle, icw, rtype, b24):
    """the frame-parallel dithered render: 66 generators x 300 and x 277 frames, neither a multiple of the
    256 threads of icw_dith_samples"""
    S = 33
    assert all((2 * S * n) % 256 for n in CALLS)
    cfg = graph.default_config(FS, need24bits=b24)
    cfg.render.render_type, cfg.render.nshape_type = rtype, abi.NSHAPE_FLAT
    cfg.render.dth_bits = 1.5
    run_case(oracle, icw, f"dithered flat render type {rtype}, 33", cfg, shift_master(), S,
             auto_k1(S, False, n_cu()))


# --------------------------------------------------------------------------- the serial graph ----
@gpu
@pytest.mark.parametrize("S", [63, 65, 129])
def test_serial_graph(oracle, icw, monkeypatch, S):
    """icw_launch_graph_serial: a lane per stream, (S + 63) / 64 waves; a Mix feeding itself is a bus-form list"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    cfg, nodes = stereo_cfg(), graph.graph_leaky_feedback()
    assert icw.graph_form(cfg, nodes) == 1
    run_case(oracle, icw, f"serial graph {S}", cfg, nodes, S, auto_k1(S, False, n_cu()))


# ----------------------------------------------------------------------------------- FP_CHECK ----
@gpu
@pytest.mark.parametrize("S", [17, 33])
def test_fp_check(oracle, icw, S):
    """icw_iir_state_fc: (n_chains + 63) / 64 waves, four chains per stream (68 and 132 chains), and the
    FP_CHECK render; inputs with NaN, +-Inf and denormals, the census of every stream compared"""
    from fpcheck_inputs import fc_cfg, special_f32
    raw = special_f32(S, sum(CALLS), seed=S)
    run_case(oracle, icw, f"FP_CHECK {S}", fc_cfg(), shift_master(), S, abi.K1_FC, raw=raw, census=True)


# -------------------------------------------------------------- subset calls on a wide context ----
@gpu
@pytest.mark.parametrize("render", ["round", "shaped"])
@pytest.mark.parametrize("mode,k1", [("plain", abi.K1_LANE), ("row", abi.K1_ROW)])
def test_subset_calls_leave_neighbours_alone(oracle, icw, monkeypatch, mode, k1, render):
    """calls over streams [f, f + cnt) of a 100-stream context, no range aligned to a group of 32 or to a
    wave of four slots: every stream outside the range -- the two beside it among them -- keeps its state
    blob byte for byte, every touched stream equals its oracle stream after every call, and the last
    full-width call checks all 100.  Once with the elementwise ROUND render (the one-stream call is then the
    one-kernel form under the row K1) and once with the serial noise-shaped one, whose generator and shaper
    state the call also addresses from its first stream on."""
    monkeypatch.setenv("ICW_K1_MODE", mode)
    S = 100
    cfg, nodes = (stereo_cfg() if render == "round" else shaped_cfg()), shift_master()
    calls = [(37, 33, 300), (0, 100, 277), (99, 1, 150), (31, 2, 201), (0, 100, 263)]
    raw = synth.batch_pcm(S, sum(n for _, _, n in calls), FS, workers=synth.cpu_workers())
    ctx = icw.Context(cfg, nodes, S)
    refs = [oracle.Stream(cfg, nodes) for _ in range(S)]
    pos = [0] * S
    t0 = time.perf_counter()
    for k, (f, cnt, n) in enumerate(calls):
        ids = list(range(f, f + cnt))
        outside = [s for s in range(S) if s < f or s >= f + cnt]
        assert all(s in outside for s in (f - 1, f + cnt) if 0 <= s < S)
        before = {s: ctx.get_state(s) for s in outside}
        seg = np.stack([raw[s, pos[s] * 4:(pos[s] + n) * 4] for s in ids])
        out, pre = ctx.process(seg, n, first=f, count=cnt, want_pre=True)
        assert ctx.last_k1_kernel() == k1, (k, ctx.last_k1_kernel())
        touched = [s for s in outside if ctx.get_state(s) != before[s]]
        assert not touched, f"call {k} over [{f}, {f + cnt}) changed the state of streams {touched[:8]}"
        ros, rps = [], []
        for i, s in enumerate(ids):
            ro, rp = refs[s].process(seg[i], n, want_pre=True)
            ros.append(ro)
            rps.append(rp)
            pos[s] += n
        got = bundle(out, pre, [ctx.meters(s) for s in ids], [ctx.n_frame(s) for s in ids])
        ref = bundle(np.stack(ros), np.stack(rps), [refs[s].meters() for s in ids], [refs[s].n_frame() for s in ids])
        assert_same(got, ref, f"{mode} K1, {render} render, call {k} over [{f}, {f + cnt})", ids)
        assert_distinct(ref["out"], got["out"], f"{mode} K1, {render} render, call {k}")
        # the streams the call left out: still at the oracle's counters
        assert [ctx.n_frame(s) for s in range(S)] == [st.n_frame() for st in refs], k
    print(f"[batch widths] subset calls, {mode} K1, {render} render: S={S} in {time.perf_counter() - t0:.2f} s")
    ctx.close()


# ------------------------------------------------------------------- the negative control (CPU) ----
def test_rig_reports_swapped_and_duplicated_streams(oracle):
    """the comparison cannot pass vacuously: against a reference with two streams swapped it names those two,
    against one whose last row is the first stream's it names the last, and the distinct-rows check names
    the doubled pair; a clean reference and NaN against NaN of the other sign pass"""
    S = 6
    cfg, nodes = stereo_cfg(), shift_master()
    raw = synth.batch_pcm(S, sum(CALLS), FS)
    ref = oracle_run(oracle, cfg, nodes, raw, CALLS)
    got = oracle_run(oracle, cfg, nodes, raw, CALLS)
    assert stream_diffs(got, ref) == [] and duplicate_rows(ref["out"]) == []
    assert len({tuple(m["clips"]) + tuple(m["peak_db"]) for m in ref["meters"]}) == S     # the meters tell streams apart

    def permuted(order):
        return bundle(ref["out"][order], ref["pre"][order], [ref["meters"][s] for s in order],
                      [ref["n_frame"][s] for s in order])
    swapped = permuted([0, 4, 2, 3, 1, 5])
    assert [s for s, _ in stream_diffs(got, swapped)] == [1, 4]
    with pytest.raises(AssertionError, match=r"2 of 6 streams differ, streams \[1, 4\]"):
        assert_same(got, swapped, "swapped")
    doubled = permuted([0, 1, 2, 3, 4, 0])
    errs = stream_diffs(got, doubled)
    assert [s for s, _ in errs] == [5] and "output bytes" in errs[0][1] and "meters" in errs[0][1]
    assert duplicate_rows(doubled["out"]) == [[0, 5]]
    with pytest.raises(AssertionError, match="share an output row"):
        assert_distinct(ref["out"], doubled["out"], "doubled")
    with pytest.raises(AssertionError, match="ORACLE"):
        assert_distinct(doubled["out"], ref["out"], "doubled reference")
    # each field on its own: one meter, one counter, one double
    for field, value in (("meters", dict(ref["meters"][3], desubnorm=ref["meters"][3]["desubnorm"] + 1)),
                         ("n_frame", ref["n_frame"][3] + 1)):
        other = dict(ref)
        other[field] = list(ref[field])
        other[field][3] = value
        assert [s for s, _ in stream_diffs(got, other)] == [3], field
    other = dict(ref, pre=ref["pre"].copy())
    other["pre"][2, 17, 1] = np.nextafter(other["pre"][2, 17, 1], np.inf)
    assert [s for s, _ in stream_diffs(got, other)] == [2]
    a, b = dict(got, pre=got["pre"].copy()), dict(ref, pre=ref["pre"].copy())
    a["pre"][2, 17, 1], b["pre"][2, 17, 1] = np.nan, -np.nan
    assert stream_diffs(a, b) == []
    # the geometry helpers, at the chip the thresholds were written down for
    assert (first_plain_width(False, 256), first_plain_width(True, 256), last_odd_row_width(256)) == (257, 513, 255)
    assert (first_lane_render_width(), last_odd_row_render_width()) == (1025, 1023)
