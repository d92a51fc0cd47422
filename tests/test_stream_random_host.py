"""CPU: the random edit sequences of tests/streamrig.py without a device.  FakeContext implements the slice of
in_cwave_amd.lib.Context that the rig calls, from one oracle.Stream per stream of its own; it answers the
refusal ops by include/icw.h's rules and the counts by counting.
  1. every plan of the GPU test's seed range runs clean through the rig: plan, model and rig agree, and the
     oracle accepts every op the generator emits;
  2. the plans cover what tests/test_gpu_stream_random.py is there for (asserted on the plans alone);
  3. a FakeContext with a planted fault is caught on one of the first 16 seeds, for every fault."""
import ctypes as C

import numpy as np
import pytest

from in_cwave_amd import abi, graph
from tests import streamrig as R
from tests.test_gpu_stream_random import SEEDS

FAULTS = ("shifted_range", "set_render_gives_depth", "unchanged_type_zeroes_rings", "advances_next_stream",
          "render_count_sticks", "row_at_6_bytes", "refused_graph_applied")


class _FakeLib:
    """the three entry points the rig calls by pointer"""

    def __init__(self, f):
        self.f = f

    def icw_set_fir_hilbert(self, h, order, beta):
        f = self.f
        # include/icw.h: refused beside per-stream lists or inputs (no icw_enable_stream_fir here), and while the
        # render or the converter count is above 1
        if order > 0 and max(f.counts()) > 1:
            return abi.EUNSUPPORTED
        raise NotImplementedError("the generator turns the FIR converter on")

    def icw_set_graph(self, h, arr, n, bypass, acc):
        from in_cwave_amd import lib as L
        f = self.f
        nodes = [arr[i] for i in range(n)]
        form = L.graph_form(f.cfg, nodes, bypass)
        nl, _, nr, nh = f.counts()
        if form == 1 and (nl > 1 or nr > 1 or nh > 1):
            if f.fault == "refused_graph_applied":
                for st in f.sts:
                    st.set_graph(nodes, bypass)
                f.lst = [(b"bus", 0)] * f.S
            return abi.EUNSUPPORTED
        raise NotImplementedError("the generator sets a list the context takes through this entry")

    def icw_process_streams(self, h, first, count, inp, in_stride, out, out_stride, n, flags, dbg, hip_stream):
        f = self.f
        if len({R.is_cw(i) for i in f.inp[first:first + count]}) > 1:
            return abi.EUNSUPPORTED
        for i in range(count):
            s = first + i
            fsz = R.frame_bytes(f.inp[s])
            raw = np.frombuffer((C.c_uint8 * (n * fsz)).from_address(inp + i * in_stride), np.uint8)
            ro, rp = f.sts[s].process(raw, n, want_pre=bool(flags & abi.F_DEBUG_PRE))
            if f.fault == "row_at_6_bytes" and ro.size == n * 4 and out_stride >= n * 6:
                ro = np.concatenate([ro, np.zeros(n * 2, np.uint8)])
            C.memmove(out + i * out_stride, ro.ctypes.data, ro.size)
            if flags & abi.F_DEBUG_PRE:
                C.memmove(dbg + i * n * 16, rp.ctypes.data, n * 16)
        s = first + count
        if f.fault == "advances_next_stream" and s < f.S and R.is_cw(f.inp[s]) == R.is_cw(f.inp[first]):
            f.sts[s].process(np.zeros(n * R.frame_bytes(f.inp[s]), np.uint8), n)
        return abi.OK


class FakeContext:
    host_only = True
    h = None

    def __init__(self, plan, oracle, fault=None):
        self.cfg, self.S, self.fault = plan.config(), plan.S, fault
        self.sts = [oracle.Stream(R.copy_cfg(self.cfg), plan.nodes()) for _ in range(plan.S)]
        self.inp = [plan.inp] * plan.S
        self.lst = [R.normal_key(plan.nodes(), plan.lst[1])] * plan.S
        self.rnd = [plan.rnd] * plan.S
        self.hil = [plan.hil] * plan.S
        self.render_entries = {plan.rnd}
        self.depth = plan.rnd[1]                # the context's own depth: icw_create's, then icw_set_outbits'
        self.cw_streams = False
        self._lib = _FakeLib(self)

    def span(self, first, count):
        if self.fault == "shifted_range":
            first = min(first + 1, self.S - 1)
            count = min(count, self.S - first)
        return range(first, first + count)

    def counts(self):
        return (len(set(self.lst)), len(set(self.inp)), len(self.render_entries), len(set(self.hil)))

    def renders_changed(self):
        """the entries no stream uses go"""
        self.render_entries |= set(self.rnd)
        if self.fault != "render_count_sticks":
            self.render_entries = set(self.rnd)

    def enable_stream_cwave(self, on=True):
        self.cw_streams = bool(on)

    def set_stream_graph(self, nodes, first=0, count=None, bypass_list=0):
        for s in self.span(first, count):
            assert self.sts[s].set_graph(nodes, bypass_list)
            self.lst[s] = R.normal_key(nodes, bypass_list)
        return True

    def set_graph(self, nodes, bypass_list=0):
        for s in range(self.S):
            assert self.sts[s].set_graph(nodes, bypass_list)
            self.lst[s] = R.normal_key(nodes, bypass_list)
        return True

    def set_stream_input(self, sample_rate, fmt, channels, first=0, count=None):
        assert self.cw_streams or (fmt not in abi.CW_FORMATS and self.cfg.in_format not in abi.CW_FORMATS), "ICW_EUNSUPPORTED"
        for s in self.span(first, count):
            self.sts[s].set_input(sample_rate, fmt, channels)
            self.inp[s] = (sample_rate, fmt, channels)

    def set_input(self, sample_rate, fmt, channels):
        self.cfg.in_format = fmt
        for s in range(self.S):
            self.sts[s].set_input(sample_rate, fmt, channels)
            self.inp[s] = (sample_rate, fmt, channels)

    def set_stream_render(self, render, need24bits, first=0, count=None):
        key = (render.dth_bits, render.quantz_type, render.render_type, render.nshape_type, render.sign_bits16, render.sign_bits24)
        for s in self.span(first, count):
            self.sts[s].set_render(render)
            self.sts[s].set_outbits(need24bits)
            self.rnd[s] = (key, int(bool(need24bits)))
        self.renders_changed()

    def set_render(self, render):
        key = (render.dth_bits, render.quantz_type, render.render_type, render.nshape_type, render.sign_bits16, render.sign_bits24)
        mixed = len(set(self.rnd)) > 1
        for s in range(self.S):
            self.sts[s].set_render(render)
            self.rnd[s] = (key, self.rnd[s][1])
            if mixed and self.fault == "set_render_gives_depth":
                self.sts[s].set_outbits(self.depth)
                self.rnd[s] = (key, self.depth)
        self.renders_changed()

    def set_outbits(self, need24bits):
        self.depth = int(bool(need24bits))
        for s in range(self.S):
            self.sts[s].set_outbits(need24bits)
            self.rnd[s] = (self.rnd[s][0], self.depth)
        self.renders_changed()

    def set_stream_hilbert(self, type_, kahan, subnorm_reject, first=0, count=None):
        for s in self.span(first, count):
            if self.fault == "unchanged_type_zeroes_rings" and self.hil[s][0] == type_:
                self.sts[s].set_hilbert_filter((type_ + 1) % 6)
            self.sts[s].set_hilbert_filter(type_)
            self.sts[s].set_hilbert_config(kahan, subnorm_reject)
            self.hil[s] = (type_, int(bool(kahan)), int(bool(subnorm_reject)))

    def set_hilbert_filter(self, type_):
        for s in range(self.S):
            self.sts[s].set_hilbert_filter(type_)
            self.hil[s] = (type_,) + self.hil[s][1:]

    def set_hilbert_config(self, kahan, subnorm_reject):
        for s in range(self.S):
            self.sts[s].set_hilbert_config(kahan, subnorm_reject)
            self.hil[s] = (self.hil[s][0], int(bool(kahan)), int(bool(subnorm_reject)))

    def stream_open(self, s, n_samples, fade_in_ms=0, fade_out_ms=0, sec_align=0, clr_nframe=0, clr_hilb=0):
        self.sts[s].open(n_samples, fade_in_ms, fade_out_ms, sec_align, clr_nframe, clr_hilb)

    def stream_reset_framecnt(self, s):
        self.sts[s].set_n_frame(0)

    def stream_graph_count(self):
        return self.counts()[0]

    def stream_input_count(self):
        return self.counts()[1]

    def stream_render_count(self):
        return self.counts()[2]

    def stream_hilbert_count(self):
        return self.counts()[3]

    def stream_render_size(self, s):
        return 3 if self.rnd[s][1] else 2

    def meters(self, s):
        return self.sts[s].meters()

    def n_frame(self, s):
        return self.sts[s].n_frame()


@pytest.fixture(scope="module")
def plans():
    return [R.make_plan(seed) for seed in range(SEEDS)]


def test_plans_are_deterministic():
    for seed in (0, 3, 17):
        a, b = R.make_plan(seed), R.make_plan(seed)
        assert [str(o) for o in a.ops] == [str(o) for o in b.ops] and (a.S, a.env, a.inp, a.rnd, a.hil) == (b.S, b.env, b.inp, b.rnd, b.hil)
        assert [R.normal_key(x, 0) for x in a.pool] == [R.normal_key(x, 0) for x in b.pool]


def test_plans_keep_the_generators_rules(plans):
    for p in plans:
        assert 1 <= p.S <= 24 or 33 <= p.S <= 70
        assert 3 <= len(p.pool) <= 5 and len({R.normal_key(x, 0) for x in p.pool}) == len(p.pool)
        calls = [o for o in p.ops if o.kind == "process"]
        assert 5 <= len(calls) <= 8 and p.ops[-1].kind == "process"
        assert sum(o.kind in R.REFUSALS for o in p.ops) <= 3
        fed = [0] * p.S
        for o in calls:
            n = o.a["n"]
            assert n in (1, 7) or 255 <= n <= 264 or 300 <= n <= 1100
            for s in range(o.a["first"], o.a["first"] + o.a["count"]):
                fed[s] += n
        assert max(fed) <= R.N_SIG


def test_every_plan_runs_clean(oracle, plans):
    for p in plans:
        R.Rig(p, FakeContext(p, oracle), oracle).run()


def survey(plans):
    """what the plans hold, from the plans alone: name -> the set of seeds (or a count of calls)"""
    seen = {}

    def plan_has(key, p):
        seen.setdefault(key, set()).add(p.seed)

    def call_has(key):
        seen[key] = seen.get(key, 0) + 1

    for p in plans:
        tab = R.Table(p)
        collapsed = set()
        hist = [[] for _ in range(p.S)]                 # every stream's channels at its calls
        for name, values in R.SWITCHES.items():
            plan_has((name, p.env.get(name)), p)
        if p.S >= 33:
            plan_has("wide", p)
        for op in p.ops:
            before = tab.counts()
            tab.apply(op)
            after = tab.counts()
            if op.kind in R.STREAM_SETTERS + R.WIDE_SETTERS + R.REFUSALS:
                plan_has(op.kind, p)
            for a, b, c in zip(R.AXES, before, after):
                if b > 1 and c == 1:
                    collapsed.add(a)
            if len(tab.kinds()) == 2:
                plan_has("both kinds", p)
            if op.kind != "process":
                continue
            for a in collapsed:
                plan_has(("collapse", a), p)
            first, count, n = op.a["first"], op.a["count"], op.a["n"]
            for s in range(first, first + count):
                if not hist[s] or hist[s][-1] != min(tab.inp[s][2], 2):
                    hist[s].append(min(tab.inp[s][2], 2))
                if hist[s][-3:] == [1, 2, 1]:
                    plan_has("mono stereo mono", p)
            if min(after) > 1:
                plan_has("all four mixed", p)
                if p.block() and n > 2 * p.block():
                    call_has("all four mixed, over two blocks")
                if op.a["device"]:
                    call_has("all four mixed, device pointers")
            here = {a: tab.count(a, first, count) > 1 for a in R.AXES}
            for i, a in enumerate(R.AXES):
                for b in R.AXES[i + 1:]:
                    if here[a] and here[b]:
                        call_has(("pair", a, b))
            cw = R.is_cw(tab.inp[first])
            if here["hilbert"] and not cw:
                kr = all(h[1] and h[2] for h in tab.hil[first:first + count])
                call_has("hilbert mixed, all Kahan + reject" if kr else "hilbert mixed, not all Kahan + reject")
            if here["render"]:
                ser = {R.is_serial(r) for r in tab.rnd[first:first + count]}
                call_has(("render mixed", "both" if len(ser) == 2 else "serial" if True in ser else "parallel"))
            if cw and len({i[1] for i in tab.inp[first:first + count]}) > 1:
                call_has("cwave formats mixed")
            if any(here.values()) and first > 0 and count < p.S:
                plan_has("subset across a boundary, first > 0", p)
            if count == 1 and max(after) > 1:
                plan_has("one stream of a mixed context", p)
    return seen


def test_coverage(plans):
    seen = survey(plans[:SEEDS])
    n = len(plans)

    def in_plans(key):
        return len(seen.get(key, ()))

    for k in R.STREAM_SETTERS + R.WIDE_SETTERS:
        assert in_plans(k) >= 8, (k, in_plans(k))
    for a in R.AXES:
        assert in_plans(("collapse", a)) >= 4, (a, in_plans(("collapse", a)))
    assert in_plans("all four mixed") >= 16, in_plans("all four mixed")
    assert seen.get("all four mixed, over two blocks", 0) >= 8
    assert seen.get("all four mixed, device pointers", 0) >= 4
    for i, a in enumerate(R.AXES):
        for b in R.AXES[i + 1:]:
            assert seen.get(("pair", a, b), 0) >= 1, (a, b)
    assert seen.get("hilbert mixed, all Kahan + reject", 0) >= 1 and seen.get("hilbert mixed, not all Kahan + reject", 0) >= 1
    for how in ("serial", "parallel", "both"):
        assert seen.get(("render mixed", how), 0) >= 1, how
    assert seen.get("cwave formats mixed", 0) >= 1
    assert in_plans("both kinds") >= 1
    assert in_plans("mono stereo mono") >= 1
    assert in_plans("subset across a boundary, first > 0") >= 16
    assert in_plans("one stream of a mixed context") >= 8
    for k in R.REFUSALS:
        assert in_plans(k) >= 4, (k, in_plans(k))
    for name, values in R.SWITCHES.items():
        for v in values:
            assert in_plans((name, v)) * 6 >= n, (name, v, in_plans((name, v)))
    assert in_plans("wide") >= 8


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught(oracle, fault):
    caught = []
    for seed in range(16):
        p = R.make_plan(seed)
        try:
            R.Rig(p, FakeContext(p, oracle, fault), oracle).run()
        except AssertionError as e:
            caught.append((seed, str(e)))
            break
    assert caught, f"no seed below 16 notices the fault {fault}"
    assert f"seed {caught[0][0]} " in caught[0][1] and " after [" in caught[0][1]
