"""The per-stream tests' shared harness (test helper): one call-and-compare, one meter check and two rigs over
the four per-stream tables of one context -- DSP lists (icw_set_stream_graph), inputs real and CWAVE
(icw_set_stream_input, icw_enable_stream_cwave), renders (icw_set_stream_render) and Hilbert converters
(icw_set_stream_hilbert).  Every comparison is bit for bit; nothing has a tolerance.

  call_streams      one icw_process_streams call and the same frames through one oracle.Stream per stream: the
                    pre-render doubles, the rendered bytes, and the guard byte past every stream's own frames.
  check_meters      clips, peak dB bits, de-subnorm counts and n_frame per stream, the FP census when asked.
                    tests/test_streamrig_compare_host.py plants deviations in both on a CPU.
  StreamRig         the hand-scripted rig of tests/test_gpu_stream_{graph,input,cwave,fir,render,hilbert}.py.
  make_plan(seed)   random edit sequences, with the context-wide setters, track opens and subset calls in
                    between; pure and deterministic: the stream count, the starting config, the environment
                    switches and the list of ops.  Nothing here touches a context or the oracle.
  Table             the settings model: per stream its input, (list, bypass), (render, depth) and converter, and
                    the four counts as include/icw.h defines them.
  Rig               runs a plan on a context (in_cwave_amd.lib.Context, or the FakeContext of
                    tests/test_stream_random_host.py, so that everything but the execution on the device is
                    checked on a CPU) and on one oracle.Stream per stream, edit by edit, and compares after
                    every op.

What a count counts (the header's words, with the doubts settled from icw_context.cpp):
  lists      distinct (normalised list, bypass flag) pairs.  prog_table_compact merges two entries when their
             compiled programs AND their node lists are bytewise equal; the program holds the bypass flag, so the
             flag belongs to the entry, and the lists are compared after amod_init's lock fan-out (graph_accept),
             so two lists that differ only in a locked right-channel field are one entry (normal_key below).
  inputs     distinct (rate, format, channels) triples (same_input).
  renders    distinct (icw_render_cfg, depth) pairs, the cfg compared field by field (same_render).
  converters distinct (type, kahan, reject) triples (same_hilb).

ICW_K1_MODE=row on a Hilbert-mixed call whose entries are not all Kahan + reject runs the lane form: the row
kernel has no baseline summation (CallPlan::pick_k1), so "forced" means row where the row form exists.

No GPU import at module level: torch and the library are imported where a call needs them."""
import ctypes as C
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from in_cwave_amd import abi, graph, synth

REAL = (abi.FMT_U8, abi.FMT_I16, abi.FMT_I24, abi.FMT_I32, abi.FMT_F32)
CW = abi.CW_FORMATS
RATES = (44100, 48000, 96000)
SWITCHES = {"ICW_K1_MODE": (None, "row", "plain"), "ICW_RENDER": (None, "serial", "row"), "ICW_BLOCK": (None, "256", "263")}
N_SIG = 8 * 1100                    # frames a plan can feed one stream: 8 calls of 1 100 at the most
NS_FIR20 = 6                        # a canned 20-tap FIR shaper (sound_render.c: icw_ns_n[6] == 20)
GUARD = 0xA5
AXES = ("list", "input", "render", "hilbert")
STREAM_SETTERS = ("set_stream_graph", "set_stream_input", "set_stream_render", "set_stream_hilbert")
WIDE_SETTERS = ("set_graph", "set_render", "set_outbits", "set_hilbert_filter", "set_hilbert_config", "set_input")
REFUSALS = ("refuse_fir", "refuse_bus_graph", "refuse_two_kinds")

# (dth_bits, quantz, render type, shaper, sign bits 16, sign bits 24), depth: ROUND + flat at 16 and 24 bit, a
# dithered flat entry (frame-parallel), dithered + MEW44 at 24 bit (serial), and a second serial entry at 16 bit
RENDER_POOL = (
    ((1.0, abi.QUANTZ_MID_TREAD, abi.RENDER_ROUND, abi.NSHAPE_FLAT, 16, 24), 0),
    ((1.0, abi.QUANTZ_MID_TREAD, abi.RENDER_ROUND, abi.NSHAPE_FLAT, 16, 24), 1),
    ((1.0, abi.QUANTZ_MID_TREAD, abi.RENDER_TPDF, abi.NSHAPE_FLAT, 16, 24), 0),
    ((1.0, abi.QUANTZ_MID_TREAD, abi.RENDER_TPDF, abi.NSHAPE_MEW44, 16, 24), 1),
    ((1.5, abi.QUANTZ_MID_RISER, abi.RENDER_GAUSS, NS_FIR20, 16, 24), 0),
)


def render_cfg(key):
    r = abi.RenderCfg()
    r.dth_bits, r.quantz_type, r.render_type, r.nshape_type, r.sign_bits16, r.sign_bits24 = key
    return r


def is_serial(render):
    """(cfg key, depth) runs the serial render: any shaper but the flat one (needs_serial)"""
    return render[0][3] != abi.NSHAPE_FLAT


def is_cw(inp):
    return inp[1] in CW


def frame_bytes(inp):
    return abi.FMT_BYTES[inp[1]] * inp[2]


def copy_cfg(cfg, **kw):
    c = abi.Config.from_buffer_copy(cfg)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def entry(rtype=abi.RENDER_ROUND, ns=abi.NSHAPE_FLAT, b24=False, quantz=abi.QUANTZ_MID_TREAD, dth=1.0, sb16=16, sb24=24):
    """a render entry as icw_set_stream_render takes it: (RenderCfg, need24bits)"""
    return render_cfg((dth, quantz, rtype, ns, sb16, sb24)), bool(b24)


def shift_list(fr):
    return [graph.master(inputs=("A",)), graph.shift(inputs=("in",), out="A", fr=fr)]


# ------------------------------------------------------------------ one call, compared ----------------------
def in_rows(raws):
    """a call's input: every stream's frames at its own frame size, in rows of the widest"""
    rows = np.zeros((len(raws), max(r.size for r in raws)), np.uint8)
    for i, r in enumerate(raws):
        rows[i, :r.size] = r
    return rows


def out_rows(n, osz, pad):
    """a call's output: rows of the widest output frame plus pad bytes, filled with the guard byte"""
    return np.full((len(osz), n * max(osz) + pad), GUARD, np.uint8)


def _stream(what, labels, first, i):
    return f"{what} stream {first + i}" + (f" {labels[i]}" if labels else "")


def call_streams(ctx, sts, first, n, raws, osz, device=False, want_pre=True, timing=False, pad=0, what="", labels=None,
                 wrapper=False):
    """one call of n frames over streams [first, first + len(raws)) -- raws[i] the frames of stream first + i,
    osz[i] its output frame size -- and the same frames through each stream's own oracle.Stream (sts[first + i]).
    Bit for bit: the pre-render doubles where asked for (as uint64, so -0.0 is not +0.0), the rendered bytes,
    their count, and the guard byte in all of the row past the stream's own frames, host and device pointers
    alike (a host_only context takes the device-pointer call with host arrays).  wrapper: the host call goes
    through ctx.process, not the entry point.  Returns the output rows.  labels[i] goes into stream
    first + i's messages"""
    count = len(raws)
    rows, out = in_rows(raws), out_rows(n, osz, pad)
    stride = out.shape[1]
    pre = np.zeros((count, n, 2), np.float64) if want_pre else None
    flags = (abi.F_DEBUG_PRE if want_pre else 0) | (abi.F_TIMING if timing else 0) | (abi.F_DEVICE_PTRS if device else 0)
    if wrapper:
        assert not device and not timing
        out, pre = ctx.process(rows, n, first=first, count=count, want_pre=want_pre, out=out)
    elif device and not getattr(ctx, "host_only", False):
        import torch
        d_in, d_out = torch.from_numpy(rows).cuda(), torch.from_numpy(out).cuda()
        d_pre = torch.zeros((count, n, 2), dtype=torch.float64, device="cuda") if want_pre else None
        torch.cuda.synchronize()
        rc = ctx._lib.icw_process_streams(ctx.h, first, count, d_in.data_ptr(), rows.shape[1], d_out.data_ptr(), stride, n,
                                          flags, d_pre.data_ptr() if want_pre else None, None)
        assert rc == abi.OK, f"{what} icw_process_streams returned {rc}"
        ctx.synchronize()
        out = d_out.cpu().numpy()
        pre = d_pre.cpu().numpy() if want_pre else None
    else:
        rc = ctx._lib.icw_process_streams(ctx.h, first, count, rows.ctypes.data, rows.shape[1], out.ctypes.data, stride, n,
                                          flags, pre.ctypes.data if want_pre else None, None)
        assert rc == abi.OK, f"{what} icw_process_streams returned {rc}"
    for i in range(count):
        w = _stream(what, labels, first, i)
        ro, rp = sts[first + i].process(raws[i], n, want_pre=want_pre)
        if want_pre:
            bad = np.flatnonzero(bits(pre[i]) != bits(rp))
            assert bad.size == 0, f"{w}: {bad.size} pre-render doubles differ, first at {bad[:4]}"
        assert ro.size == n * osz[i], f"{w}: the oracle rendered {ro.size} bytes, {n} frames of {osz[i]} are {n * osz[i]}"
        bad = np.flatnonzero(out[i, :ro.size] != ro)
        assert bad.size == 0, f"{w}: {bad.size} rendered bytes differ, first at {bad[:4]}"
        bad = np.flatnonzero(out[i, ro.size:] != GUARD)
        assert bad.size == 0, f"{w}: {bad.size} bytes written past its {ro.size} bytes of frames, first at {ro.size + bad[:4]}"
    return out


def check_meters(ctx, sts, what="", census=False, first=0, labels=None):
    """clips, peak dB bits, de-subnorm counts and n_frame of streams [first, first + len(sts)) against their
    oracle streams sts, and the FP census when asked"""
    for i, st in enumerate(sts):
        s, w = first + i, _stream(what, labels, first, i)
        m, r = ctx.meters(s), st.meters()
        assert m["clips"] == r["clips"], f"{w}: clips {m} vs {r}"
        assert bits(np.array(m["peak_db"])).tolist() == bits(np.array(r["peak_db"])).tolist(), f"{w}: peaks {m} vs {r}"
        assert m["desubnorm"] == r["desubnorm"], f"{w}: de-subnorm count {m} vs {r}"
        assert ctx.n_frame(s) == st.n_frame(), f"{w}: n_frame {ctx.n_frame(s)} vs {st.n_frame()}"
        if census:
            assert np.array_equal(ctx.fp_census(s), st.fp_census()), f"{w}: FP census"


def normal_key(nodes, bypass):
    """a list as the context stores it: amod_init's L/R lock fan-out (graph_accept) applied, with the flag"""
    out = []
    for n in nodes:
        t = abi.Node.from_buffer_copy(n)
        if t.lock_gain:
            t.gain[1], t.iq_invert[1] = t.gain[0], t.iq_invert[0]
        if t.mode == abi.MODE_SHIFT and t.lock_shift:
            t.fr_shift[1] = -t.fr_shift[0] if t.sign_lock_shift else t.fr_shift[0]
            t.is_shift[1] = t.is_shift[0]
        if t.mode == abi.MODE_PM:
            if t.lock_freq:
                t.pm_freq[1], t.is_pm[1] = t.pm_freq[0], t.is_pm[0]
            if t.lock_phase:
                t.pm_phase[1] = t.pm_phase[0]
            if t.lock_level:
                t.pm_level[1] = t.pm_level[0]
            if t.lock_angle:
                t.pm_angle[1] = t.pm_angle[0]
        out.append(bytes(t))
    return b"".join(out), int(bool(bypass))


@lru_cache(maxsize=512)
def signal(s, inp, silent=False):
    """stream s's test signal at an input: synth.stream_pcm, synth.stream_cwave for the CWAVE formats (as
    StreamRig.signal makes it); a silent stream is fed digital silence"""
    rate, fmt, ch = inp
    gen = synth.stream_cwave if fmt in CW else synth.stream_pcm
    raw = gen(s, N_SIG, rate, channels=ch, fmt=fmt)
    if silent:
        raw = np.zeros_like(raw) if fmt != abi.FMT_U8 else np.full_like(raw, 128)
    raw.setflags(write=False)
    return raw


# ------------------------------------------------------------------ the plan --------------------------------
@dataclass
class Op:
    kind: str
    a: dict = field(default_factory=dict)

    def __str__(self):
        def short(v):
            if isinstance(v, tuple) and v and isinstance(v[0], tuple):
                return "(type=%d ns=%d, %d bit)" % (v[0][2], v[0][3], 24 if v[1] else 16)
            return str(v)
        return self.kind + "(" + ", ".join(f"{k}={short(v)}" for k, v in self.a.items()) + ")"


@dataclass
class Plan:
    seed: int
    S: int
    env: dict                       # switch -> value, unset ones left out
    cwave: bool                     # icw_enable_stream_cwave at creation
    frmod_scaled: int
    inp: tuple                      # the starting (rate, format, channels)
    lst: tuple                      # (pool index, bypass)
    rnd: tuple                      # (cfg key, depth)
    hil: tuple                      # (type, kahan, reject)
    pool: list                      # 3-5 distinct register-form lists
    silent: frozenset
    ops: list

    def config(self):
        cfg = graph.default_config(self.inp[0], fmt=self.inp[1], channels=self.inp[2], need24bits=bool(self.rnd[1]),
                                   hilbert_type=self.hil[0])
        cfg.iir_kahan, cfg.iir_subnorm_reject = self.hil[1], self.hil[2]
        cfg.frmod_scaled = self.frmod_scaled
        cfg.bypass_list = self.lst[1]
        cfg.render = render_cfg(self.rnd[0])
        return cfg

    def nodes(self):
        return self.pool[self.lst[0]]

    def block(self):
        """frames per launch block, None for the library's own (far above any call here)"""
        return int(self.env["ICW_BLOCK"]) if "ICW_BLOCK" in self.env else None

    def where(self):
        return f"seed {self.seed} S={self.S} {self.env or 'no switches'}{' cwave' if self.cwave else ''}"


class Table:
    """the settings in force, per stream, and the counts"""

    def __init__(self, plan):
        S = plan.S
        self.S, self.pool = S, plan.pool
        self.inp = [plan.inp] * S
        self.lst = [plan.lst] * S
        self.rnd = [plan.rnd] * S
        self.hil = [plan.hil] * S
        self._keys = {}

    def list_key(self, l):
        if l not in self._keys:
            self._keys[l] = normal_key(self.pool[l[0]], l[1]) if l[0] >= 0 else (b"bus", 0)
        return self._keys[l]

    def axis(self, name):
        return {"list": [self.list_key(l) for l in self.lst], "input": self.inp, "render": self.rnd, "hilbert": self.hil}[name]

    def count(self, name, first=0, count=None):
        v = self.axis(name)
        return len(set(v[first:self.S if count is None else first + count]))

    def counts(self):
        return tuple(self.count(a) for a in AXES)

    def kinds(self, first=0, count=None):
        return {is_cw(i) for i in self.inp[first:self.S if count is None else first + count]}

    def segments(self):
        """maximal ranges of consecutive streams of one kind, as (first, count)"""
        out, s = [], 0
        while s < self.S:
            n = 1
            while s + n < self.S and is_cw(self.inp[s + n]) == is_cw(self.inp[s]):
                n += 1
            out.append((s, n))
            s += n
        return out

    def apply(self, op):
        """an edit op's effect on the settings (refusals and track ops change none)"""
        a, k = op.a, op.kind
        r = range(a["first"], a["first"] + a["count"]) if "first" in a and k in STREAM_SETTERS else range(self.S)
        for s in r:
            if k in ("set_stream_graph", "set_graph"):
                self.lst[s] = (a["li"], a["bypass"])
            elif k in ("set_stream_input", "set_input"):
                self.inp[s] = a["inp"]
            elif k == "set_stream_render":
                self.rnd[s] = a["render"]
            elif k == "set_render":
                self.rnd[s] = (a["cfg"], self.rnd[s][1])
            elif k == "set_outbits":
                self.rnd[s] = (self.rnd[s][0], a["b24"])
            elif k == "set_stream_hilbert":
                self.hil[s] = a["hil"]
            elif k == "set_hilbert_filter":
                self.hil[s] = (a["type"],) + self.hil[s][1:]
            elif k == "set_hilbert_config":
                self.hil[s] = (self.hil[s][0], a["kahan"], a["reject"])


def _pool(rng, cfg):
    """3-5 lists, distinct as the context compares them, each in the register form with the flag off (with
    it on only the Master runs: the register form whatever follows).  Built as register_list of
    tests/test_gpu_stream_graph.py builds them; the graph.* canned lists are members now and then"""
    from in_cwave_amd import lib as L
    from tests.test_gpu_stream_graph import register_list
    want = int(rng.integers(3, 6))
    canned = [graph.graph_shift_master, graph.graph_master_only, graph.graph_pm_shift_mix]
    pool, keys = [], set()
    for k in rng.permutation(3)[:int(rng.integers(0, 3))]:
        pool.append(canned[int(k)]())
        keys.add(normal_key(pool[-1], 0))
    while len(pool) < want:
        nodes = register_list(L, cfg, rng, 0, want_chain=None if rng.random() < 0.5 else bool(rng.random() < 0.5))
        if normal_key(nodes, 0) not in keys:
            keys.add(normal_key(nodes, 0))
            pool.append(nodes)
    return pool


def _draw_range(rng, S):
    """[first, first + count): the whole batch now and then, one stream, else any range"""
    r = rng.random()
    if r < 0.12:
        return 0, S
    if r < 0.3:
        return int(rng.integers(0, S)), 1
    first = int(rng.integers(0, S))
    return first, int(rng.integers(1, S - first + 1))


def _draw_input(rng, cwave, p_cw=0.45):
    fmts = CW if cwave and rng.random() < p_cw else REAL
    return int(rng.choice(RATES)), int(rng.choice(fmts)), int(rng.integers(1, 3))


def _draw_hilbert(rng, kr_bias):
    if rng.random() < kr_bias:
        return int(rng.integers(0, 6)), 1, 1
    return int(rng.integers(0, 6)), int(rng.integers(0, 2)), int(rng.integers(0, 2))


def _draw_n(rng):
    r = rng.random()
    if r < 0.06:
        return 1
    if r < 0.13:
        return 7
    if r < 0.35:
        return int(rng.integers(255, 265))
    return int(rng.integers(300, 1101))


def _stream_setter(rng, plan_bits, tab, axis):
    cwave, kr_bias = plan_bits
    first, count = _draw_range(rng, tab.S)
    a = {"first": first, "count": count}
    if axis == "list":
        a.update(li=int(rng.integers(0, len(tab.pool))), bypass=int(rng.random() < 0.15))
        return Op("set_stream_graph", a)
    if axis == "input":
        cur = tab.inp[first]
        if rng.random() < 0.35 and not is_cw(cur):
            a["inp"] = (cur[0], cur[1], 3 - min(cur[2], 2))       # the same track format, mono <-> stereo
        else:
            a["inp"] = _draw_input(rng, cwave)
        return Op("set_stream_input", a)
    if axis == "render":
        a["render"] = RENDER_POOL[int(rng.integers(0, len(RENDER_POOL)))]
        return Op("set_stream_render", a)
    a["hil"] = _draw_hilbert(rng, kr_bias)
    return Op("set_stream_hilbert", a)


def _wide_setter(rng, plan_bits, tab, kind):
    cwave, kr_bias = plan_bits
    if kind == "set_graph":
        return Op(kind, {"li": int(rng.integers(0, len(tab.pool))), "bypass": int(rng.random() < 0.15)})
    if kind == "set_render":
        return Op(kind, {"cfg": RENDER_POOL[int(rng.choice([0, 2, 3, 3, 4]))][0]})
    if kind == "set_outbits":
        return Op(kind, {"b24": int(rng.integers(0, 2))})
    if kind == "set_hilbert_filter":
        return Op(kind, {"type": int(rng.integers(0, 6))})
    if kind == "set_hilbert_config":
        k, r = (1, 1) if rng.random() < 0.5 else (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
        return Op(kind, {"kahan": k, "reject": r})
    # without the opt-in a context whose input is CWAVE takes no per-stream input: real formats only there
    return Op("set_input", {"inp": _draw_input(rng, cwave, 0.3)})


def _runs(values, first, count):
    """boundaries b in (first, first + count) where values[b] != values[b - 1]"""
    return [b for b in range(first + 1, first + count) if values[b] != values[b - 1]]


def _draw_call_range(rng, tab):
    """whole batch, across run boundaries, inside one run, or one stream -- inside one kind"""
    segs = tab.segments()
    f0, n0 = segs[int(rng.choice(len(segs), p=np.array([n for _, n in segs]) / tab.S))]
    r = rng.random()
    if r < 0.3 or n0 == 1:
        return f0, n0
    every = list(zip(*(tab.axis(a) for a in AXES)))
    if r < 0.68:
        axes = [a for a in AXES if _runs(tab.axis(a), f0, n0)]
        if axes:
            bs = _runs(tab.axis(str(rng.choice(axes))), f0, n0)
            b = int(rng.choice(bs))
            lo = int(rng.integers(max(f0, b - 4), b))
            if lo == 0 and b > 1 and rng.random() < 0.7:
                lo = int(rng.integers(1, b))
            hi = int(rng.integers(b + 1, min(f0 + n0, b + 5) + 1))
            return lo, hi - lo
    if r < 0.82:
        bs = [f0] + _runs(every, f0, n0) + [f0 + n0]
        long = [(bs[i], bs[i + 1] - bs[i]) for i in range(len(bs) - 1) if bs[i + 1] - bs[i] >= 2]
        if long:
            f, n = long[int(rng.integers(0, len(long)))]
            c = int(rng.integers(1, n + 1))
            return f + int(rng.integers(0, n - c + 1)), c
    return f0 + int(rng.integers(0, n0)), 1


def make_plan(seed):
    """the plan of a seed: pure, deterministic, no context and no oracle"""
    rng = np.random.default_rng(977_003 * seed + 41)
    S = int(rng.integers(33, 71)) if seed % 6 == 3 else int(rng.integers(1, 25))
    env = {}
    for name, values in SWITCHES.items():
        v = values[int(rng.integers(0, 3))]
        if v is not None:
            env[name] = v
    cwave = bool(rng.random() < 0.4)
    kr_bias = 0.85 if rng.random() < 0.55 else 0.0
    bits_ = (cwave, kr_bias)
    inp = _draw_input(rng, cwave, 0.5)
    hil = (1, 1, 1) if rng.random() < 0.6 else _draw_hilbert(rng, kr_bias)
    rnd = RENDER_POOL[0] if rng.random() < 0.6 else RENDER_POOL[int(rng.integers(0, len(RENDER_POOL)))]
    plan = Plan(seed=seed, S=S, env=env, cwave=cwave, frmod_scaled=int(rng.random() < 0.6), inp=inp, lst=(0, 0), rnd=rnd,
                hil=hil, pool=[], silent=frozenset(s for s in range(S) if rng.random() < 0.15), ops=[])
    plan.pool = _pool(rng, plan.config())
    plan.lst = (int(rng.integers(0, len(plan.pool))), int(rng.random() < 0.1))
    tab, ops = Table(plan), plan.ops
    want_refusal = {k: bool(rng.random() < 0.55) for k in REFUSALS}

    def emit(op):
        ops.append(op)
        tab.apply(op)

    def refusals():
        nl, ni, nr, nh = tab.counts()
        if want_refusal["refuse_fir"] and (nr > 1 or nh > 1):
            want_refusal["refuse_fir"] = False
            emit(Op("refuse_fir"))
        if want_refusal["refuse_bus_graph"] and (nl > 1 or nr > 1 or nh > 1):
            want_refusal["refuse_bus_graph"] = False
            emit(Op("refuse_bus_graph"))
        if want_refusal["refuse_two_kinds"] and len(tab.kinds()) == 2:
            want_refusal["refuse_two_kinds"] = False
            segs = tab.segments()
            k = int(rng.integers(0, len(segs) - 1))
            lo = int(rng.integers(segs[k][0], segs[k][0] + segs[k][1]))
            hi = int(rng.integers(segs[k + 1][0] + 1, segs[k + 1][0] + segs[k + 1][1] + 1))
            emit(Op("refuse_two_kinds", {"first": lo, "count": hi - lo, "n": int(rng.integers(1, 300))}))

    def edit():
        r = rng.random()
        if r < 0.66:
            emit(_stream_setter(rng, bits_, tab, str(rng.choice(AXES))))
        elif r < 0.86:
            emit(_wide_setter(rng, bits_, tab, str(rng.choice(WIDE_SETTERS))))
        elif r < 0.96:
            emit(Op("stream_open", {"s": int(rng.integers(0, S)), "n": 0, "fade_in_ms": int(rng.choice([0, 5, 20])),
                                    "fade_out_ms": int(rng.choice([0, 5, 20])), "clr_nframe": int(rng.integers(0, 2)),
                                    "clr_hilb": int(rng.integers(0, 2)), "extra": int(rng.choice([0, 0, int(rng.integers(1, 400))]))}))
        else:
            emit(Op("stream_reset_framecnt", {"s": int(rng.integers(0, S))}))

    if rng.random() < 0.85:                             # a mixed context before the first call, most of the time
        for axis in AXES:
            if rng.random() < 0.8:
                for _ in range(int(rng.integers(1, 4))):
                    emit(_stream_setter(rng, bits_, tab, axis))
    for call in range(int(rng.integers(5, 9))):
        for _ in range(int(rng.integers(0 if call == 0 else 1, 4))):
            edit()
        refusals()
        first, count = _draw_call_range(rng, tab)
        emit(Op("process", {"first": first, "count": count, "n": _draw_n(rng), "device": bool(rng.random() < 0.33),
                            "want_pre": bool(rng.random() >= 0.33)}))
    # every track ends at or after the last frame the plan feeds that stream: the frames fed until the stream's
    # next open (or the end), and `extra` beyond them
    for i, op in enumerate(ops):
        if op.kind != "stream_open":
            continue
        s, fed = op.a["s"], 0
        for later in ops[i + 1:]:
            if later.kind == "stream_open" and later.a["s"] == s:
                break
            if later.kind == "process" and later.a["first"] <= s < later.a["first"] + later.a["count"]:
                fed += later.a["n"]
        op.a["n"] = fed + op.a.pop("extra")
    return plan


# ------------------------------------------------------------------ the rig ---------------------------------
class Rig:
    """a plan on a context and on one oracle.Stream per stream.  ctx is what the plan's config, list and stream
    count create (the caller sets the switches first: they are read at icw_create); host_only contexts take the
    device-pointer calls with host arrays.  after_call(rig, op) runs after every process call"""

    def __init__(self, plan, ctx, oracle, after_call=None):
        self.plan, self.ctx, self.after_call = plan, ctx, after_call
        cfg = plan.config()
        self.sts = [oracle.Stream(copy_cfg(cfg), plan.nodes()) for _ in range(plan.S)]
        self.tab = Table(plan)
        self.t = [0] * plan.S
        self.log = []
        if plan.cwave:
            ctx.enable_stream_cwave()

    def where(self, op=None):
        return f"{self.plan.where()} after [{'; '.join(self.log)}]" + (f" at {op}" if op else "")

    def raw(self, s, n):
        f = frame_bytes(self.tab.inp[s])
        return signal(s, self.tab.inp[s], s in self.plan.silent)[self.t[s] * f:(self.t[s] + n) * f]

    def run(self):
        self.check_tables(None)
        for op in self.plan.ops:
            getattr(self, "op_" + ("edit" if op.kind in STREAM_SETTERS + WIDE_SETTERS else op.kind))(op)
            self.log.append(str(op))
        return self

    def check_tables(self, op):
        ctx, tab = self.ctx, self.tab
        got = (ctx.stream_graph_count(), ctx.stream_input_count(), ctx.stream_render_count(), ctx.stream_hilbert_count())
        assert got == tab.counts(), f"{self.where(op)}: (list, input, render, converter) counts {got}, the model has {tab.counts()}"
        sizes = [ctx.stream_render_size(s) for s in range(tab.S)]
        want = [3 if r[1] else 2 for r in tab.rnd]
        assert sizes == want, f"{self.where(op)}: stream_render_size {sizes}, the model has {want}"

    # -- edits: the setter on the context, the reference's own calls on the oracles
    def op_edit(self, op):
        a, k, ctx = op.a, op.kind, self.ctx
        sts = self.sts[a["first"]:a["first"] + a["count"]] if k in STREAM_SETTERS else self.sts
        if k in ("set_stream_graph", "set_graph"):
            nodes = self.plan.pool[a["li"]]
            ok = ctx.set_stream_graph(nodes, a["first"], a["count"], a["bypass"]) if k == "set_stream_graph" else ctx.set_graph(nodes, a["bypass"])
            assert ok, self.where(op)
            for st in sts:
                assert st.set_graph(nodes, a["bypass"]), self.where(op)
        elif k in ("set_stream_input", "set_input"):
            if k == "set_input":
                ctx.set_input(*a["inp"])
            else:
                ctx.set_stream_input(*a["inp"], first=a["first"], count=a["count"])
            for st in sts:
                st.set_input(*a["inp"])
        elif k == "set_stream_render":
            r = render_cfg(a["render"][0])
            ctx.set_stream_render(r, a["render"][1], a["first"], a["count"])
            for st in sts:
                st.set_render(r)
                st.set_outbits(a["render"][1])
        elif k == "set_render":
            r = render_cfg(a["cfg"])
            ctx.set_render(r)
            for st in sts:
                st.set_render(r)
        elif k == "set_outbits":
            ctx.set_outbits(a["b24"])
            for st in sts:
                st.set_outbits(a["b24"])
        elif k == "set_stream_hilbert":
            ctx.set_stream_hilbert(*a["hil"], first=a["first"], count=a["count"])
            for st in sts:
                st.set_hilbert_filter(a["hil"][0])
                st.set_hilbert_config(a["hil"][1], a["hil"][2])
        elif k == "set_hilbert_filter":
            ctx.set_hilbert_filter(a["type"])
            for st in sts:
                st.set_hilbert_filter(a["type"])
        elif k == "set_hilbert_config":
            ctx.set_hilbert_config(a["kahan"], a["reject"])
            for st in sts:
                st.set_hilbert_config(a["kahan"], a["reject"])
        else:
            raise ValueError(k)
        self.tab.apply(op)
        self.check_tables(op)

    def op_stream_open(self, op):
        a = op.a
        self.ctx.stream_open(a["s"], a["n"], a["fade_in_ms"], a["fade_out_ms"], 0, a["clr_nframe"], a["clr_hilb"])
        self.sts[a["s"]].open(a["n"], a["fade_in_ms"], a["fade_out_ms"], 0, a["clr_nframe"], a["clr_hilb"])
        self.check_tables(op)

    def op_stream_reset_framecnt(self, op):
        self.ctx.stream_reset_framecnt(op.a["s"])
        self.sts[op.a["s"]].set_n_frame(0)
        self.check_tables(op)

    # -- refusals: ICW_EUNSUPPORTED, and nothing changes (the tables now, the streams by going on)
    def op_refuse_fir(self, op):
        rc = self.ctx._lib.icw_set_fir_hilbert(self.ctx.h, 64, 8.0)
        assert rc == abi.EUNSUPPORTED, f"{self.where(op)}: icw_set_fir_hilbert returned {rc}"
        self.check_tables(op)

    def op_refuse_bus_graph(self, op):
        bus = graph.graph_feedback_pm_shift()
        acc = C.c_int()
        rc = self.ctx._lib.icw_set_graph(self.ctx.h, graph.node_array(bus), len(bus), 0, C.byref(acc))
        assert rc == abi.EUNSUPPORTED, f"{self.where(op)}: icw_set_graph with a bus-form list returned {rc}"
        self.check_tables(op)

    def op_refuse_two_kinds(self, op):
        a = op.a
        span = range(a["first"], a["first"] + a["count"])
        rows, out = in_rows([self.raw(s, a["n"]) for s in span]), out_rows(a["n"], [self.osz(s) for s in span], 0)
        rc = self.ctx._lib.icw_process_streams(self.ctx.h, a["first"], a["count"], rows.ctypes.data, rows.shape[1], out.ctypes.data,
                                               out.shape[1], a["n"], 0, None, None)
        assert rc == abi.EUNSUPPORTED, f"{self.where(op)}: a call over real and CWAVE streams returned {rc}"
        assert (out == GUARD).all(), f"{self.where(op)}: the refused call wrote output"
        self.check_tables(op)

    # -- calls
    def osz(self, s):
        return 6 if self.tab.rnd[s][1] else 4

    def op_process(self, op):
        a, tab = op.a, self.tab
        first, count, n = a["first"], a["count"], a["n"]
        where, span = self.where(op), range(a["first"], a["first"] + a["count"])
        labels = [f"(input {tab.inp[s]}, list {tab.lst[s]}, render {tab.rnd[s][0][2:4]} / {24 if tab.rnd[s][1] else 16} bit, "
                  f"converter {tab.hil[s]}) from frame {self.t[s]}" for s in span]
        call_streams(self.ctx, self.sts, first, n, [self.raw(s, n) for s in span], [self.osz(s) for s in span], device=a["device"],
                     want_pre=a["want_pre"], pad=(self.plan.seed + len(self.log)) % 3, what=where + ":", labels=labels)
        for s in span:
            self.t[s] += n
        check_meters(self.ctx, self.sts[first:first + count], where + ":", first=first, labels=labels)
        if self.after_call:
            self.after_call(self, op)


class StreamRig:
    """a hand-scripted context with one oracle.Stream and one test signal per stream, beside the plan-driven Rig.
    Stream s runs lists[s] (bypass[s]), reads inputs[s] = (rate, fmt, channels), renders with renders[s] =
    (RenderCfg, need24bits) and converts with settings[s] = (type, kahan, reject); a missing table or a None entry
    is the context's own: cfg's, and the list `nodes` (lists[0] where not given).  silent: streams fed digital
    silence; cwave: icw_enable_stream_cwave first; sig0: the first stream's signal seed; pad: the bytes step adds to
    a call's output rows unless told otherwise.  Every stream keeps its own frame position t[s]"""

    def __init__(self, icw, oracle, cfg, n_total, S=None, nodes=None, lists=None, bypass=None, inputs=None, renders=None,
                 settings=None, silent=(), cwave=False, sig0=0, pad=0):
        S = len(next(x for x in (lists, inputs, renders, settings, [None] * (S or 0)) if x is not None))
        own = (cfg.hilbert_type, cfg.iir_kahan, cfg.iir_subnorm_reject)
        lists, settings = lists or [None] * S, settings or [None] * S
        nodes = nodes or lists[0] or graph.graph_shift_master()
        lists = [nodes if nl is None else nl for nl in lists]
        self.pad = pad
        self.ctx = icw.Context(copy_cfg(cfg), nodes, S)
        if cwave:
            self.ctx.enable_stream_cwave()
        self.sts = []
        for s in range(S):
            byp = bypass[s] if bypass else cfg.bypass_list
            t, k, r = settings[s] or own
            self.sts.append(oracle.Stream(copy_cfg(cfg, bypass_list=byp, hilbert_type=t, iir_kahan=k, iir_subnorm_reject=r), lists[s]))
            if lists[s] is not nodes or byp != cfg.bypass_list:
                assert self.ctx.set_stream_graph(lists[s], s, 1, byp)
        self.cur = [own] * S
        self.inputs = [(cfg.sample_rate, cfg.in_format, cfg.in_channels)] * S
        for s, inp in enumerate(inputs or []):
            if inp is not None:
                self.set_input(s, *inp)
        self.raw = [self.signal(sig0 + s, n_total, *inp) for s, inp in enumerate(self.inputs)]
        for s in silent:
            self.raw[s] = np.full_like(self.raw[s], 128 if self.inputs[s][1] == abi.FMT_U8 else 0)
        self.osz = [2 * self.ctx.stream_render_size(s) for s in range(S)]
        for s, e in enumerate(renders or []):
            if e is not None:
                self.set_render(s, e)
        # runs of equal settings go in one call of the setter each; the oracles were created with theirs
        s = 0
        while s < S:
            n = 1
            while s + n < S and settings[s + n] == settings[s]:
                n += 1
            if settings[s] is not None:
                self.ctx.set_stream_hilbert(*settings[s], first=s, count=n)
                self.cur[s:s + n] = [settings[s]] * n
            s += n
        self.t = [0] * S

    @staticmethod
    def signal(seed, n, rate, fmt, ch):
        """synth.stream_cwave's analytic signal for the CWAVE formats, synth.stream_pcm's for the real ones"""
        return (synth.stream_cwave if fmt in CW else synth.stream_pcm)(seed, n, rate, channels=ch, fmt=fmt)

    # -- edits over streams [s, s + count): the setter on the context, the reference's own calls on the oracles
    def set_graph(self, s, nodes, count=1, bypass=0):
        assert self.ctx.set_stream_graph(nodes, s, count, bypass)
        for st in self.sts[s:s + count]:
            assert st.set_graph(nodes, bypass)

    def set_input(self, s, rate, fmt, ch, count=1):
        self.ctx.set_stream_input(rate, fmt, ch, s, count)
        for i in range(s, s + count):
            self.sts[i].set_input(rate, fmt, ch)
            self.inputs[i] = (rate, fmt, ch)

    def set_render(self, s, e, count=1):
        r, b24 = e
        self.ctx.set_stream_render(r, b24, s, count)
        for i in range(s, s + count):
            self.sts[i].set_render(r)
            self.sts[i].set_outbits(b24)
            self.osz[i] = 6 if b24 else 4
            assert self.ctx.stream_render_size(i) == (3 if b24 else 2)

    def set_hilbert(self, s, e, count=1):
        """hq_rp_create / iir_rp_setcfg on the oracles"""
        self.ctx.set_stream_hilbert(*e, first=s, count=count)
        for i in range(s, s + count):
            self.sts[i].set_hilbert_filter(e[0])
            self.sts[i].set_hilbert_config(e[1], e[2])
            self.cur[i] = e

    # -- calls
    def fsz(self, s):
        return abi.FMT_BYTES[self.inputs[s][1]] * self.inputs[s][2]

    def frames(self, s, n, t=None):
        t, f = self.t[s] if t is None else t, self.fsz(s)
        return self.raw[s][t * f:(t + n) * f]

    def rows(self, n, first, count, t=None):
        """a call's input rows: every stream's n frames from its own position (from frame t, if given)"""
        return in_rows([self.frames(first + i, n, t) for i in range(count)])

    def step(self, n, first=0, count=None, device=False, what="", timing=False, pad=None, want_pre=True, advance=True,
             wrapper=False):
        """one call over streams [first, first + count), every stream checked against its oracle (call_streams);
        advance=False leaves the frame positions where they are.  Returns the output rows"""
        count = len(self.sts) - first if count is None else count
        span = range(first, first + count)
        labels = [f"{self.inputs[s]} converter {self.cur[s]} from frame {self.t[s]}" for s in span]
        out = call_streams(self.ctx, self.sts, first, n, [self.frames(s, n) for s in span], self.osz[first:first + count],
                           device=device, want_pre=want_pre, timing=timing, pad=self.pad if pad is None else pad, what=what,
                           labels=labels, wrapper=wrapper)
        if advance:
            for s in span:
                self.t[s] += n
        return out

    def check(self, what="", census=False):
        check_meters(self.ctx, self.sts, what, census)

    def close(self):
        self.ctx.close()
