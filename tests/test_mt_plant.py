"""The planted MT19937 states of tests/mtplant.py, no GPU.

The twist and its inverse are checked against numpy.random.RandomState (the same MT19937) fed the same
state; the planted words are where they were asked for up to 120 twists ahead, the pair that straddles
a twist included; and the oracle, handed a planted state through Stream.set_mt, renders what the
independent pure-Python restatement (tests/pyref_chain.py) renders with the rejection three to five
twists ahead -- which pins the oracle's rejection path beyond the current 624 words, the stretch the
forced rejections of test_gpu_dither_flat.py stay within.  A negative control shows that the planted
pair is what the bytes depend on.
"""
import numpy as np
import pytest

import mtplant
from mtplant import N


def _state(seed):
    """a state as init_genrand leaves it after some use: RandomState's own words and position"""
    rs = np.random.RandomState(seed)
    rs.bytes(4 * (700 + 2 * seed))
    _, words, pos = rs.get_state()[:3]
    return words.astype(np.uint32), int(pos)


def _numpy_words(words, idx, n):
    rs = np.random.RandomState(0)
    rs.set_state(("MT19937", np.asarray(words, dtype=np.uint32), int(idx)))
    return np.frombuffer(rs.bytes(4 * n), dtype="<u4")


def test_twist_is_numpys_and_untwist_undoes_it():
    for seed in range(4):
        s, idx = _state(seed)
        assert np.array_equal(mtplant.words_from(s, idx, 5000), _numpy_words(s, idx, 5000))
        t = mtplant.twist(s)
        u = mtplant.untwist(t)
        assert np.array_equal(u[1:], s[1:]) and (u[0] ^ s[0]) & mtplant.HI == 0
        # the low bits of word 0 are read by nothing, and the walked-back array is a twist output itself
        assert np.array_equal(mtplant.twist(u), t)
        assert np.array_equal(mtplant.twist(mtplant.untwist(u)), u)
        k = s
        for _ in range(45):
            k = mtplant.twist(k)
        b = k
        for _ in range(45):
            b = mtplant.untwist(b)
        assert np.array_equal(b[1:], s[1:])


@pytest.mark.parametrize("k", [0, 1, 2, 7, 45, 119, 120])
@pytest.mark.parametrize("where", ["mid", "start", "end", "straddle", "two"])
def test_planted_words_are_where_asked(k, where):
    s, idx = _state(k % 5)
    if where == "straddle":
        idx |= 1                                   # pairs are aligned to the call's start: odd idx for 623 | 0
        base = (k + 1) * N - 1 - idx
        offs = [base, base + 1]
    elif where == "start":
        base = k * N - idx if k else 0
        base += base & 1
        offs = [base, base + 1]
    elif where == "end":
        base = (k + 1) * N - 2 - idx
        base -= base & 1
        offs = [base, base + 1]
    elif where == "two":                           # two pairs of one generation, one value between them
        base = k * N + 300 - idx
        base += base & 1
        offs = [base, base + 1, base + 4, base + 5]
    else:
        base = k * N + 100 - idx
        base += base & 1
        offs = [base, base + 1]
    assert min(offs) >= 0
    w = mtplant.plant(s, idx, offs)
    n = max(offs) + 700
    got = _numpy_words(w, idx, n)                  # numpy's generator on the planted state
    assert all(got[o] == 0 for o in offs)
    assert np.array_equal(got, mtplant.words_from(w, idx, n))
    # the model of the draws takes each as a pair, in the sample asked for (W = 2: sample = pair)
    rej, starts = mtplant.consumption(w, idx, 2, n // 2 - 40)
    assert [o for _, o in rej] == offs[0::2]
    assert [t for t, _ in rej] == [o // 2 - i for i, o in enumerate(offs[0::2])]
    # the generations in between keep the words the state would have reached anyway, but for the few words
    # the constraints take
    g = (idx + offs[0]) // N
    a, b = s, w
    for _ in range(g):
        a, b = mtplant.twist(a), mtplant.twist(b)
    assert np.count_nonzero(a != b) <= len(offs) + 2


def test_plant_refuses_what_it_cannot_place():
    s, idx = _state(1)
    with pytest.raises(ValueError):
        mtplant.plant(s, idx, [10, 11, 10 + 3 * N, 11 + 3 * N])


def _render_cfg(rtype, nshape=2):
    from in_cwave_amd import abi, graph
    cfg = graph.default_config(44100, fmt=abi.FMT_I16, channels=2)
    cfg.render.render_type, cfg.render.nshape_type = rtype, nshape
    cfg.render.dth_bits = 1.5
    return cfg, [graph.master(gain=1.0)]


W_OF = {1: 2, 2: 4, 3: 2, 4: 24}                    # RPDF, TPDF, STPDF, GAUSS: words per sample


def _planted_pair(oracle, rtype, n0, twists):
    """an oracle stream and a pure-Python one after n0 frames, both handed the same planted states: L with
    a pair `twists[0]` twists ahead, R with the pair straddling twist `twists[1]`"""
    from in_cwave_amd import synth
    from pyref_chain import PyStream
    cfg, nodes = _render_cfg(rtype)
    W = W_OF[rtype]
    n = (twists[1] + 2) * N // W + 40
    raw = synth.stream_pcm(11 + rtype, n0 + n, 44100)
    st, py = oracle.Stream(cfg, nodes), PyStream(cfg, nodes)
    o0, _ = st.process(raw[:n0 * 4], n0)
    p0, _ = py.process(raw[:n0 * 4], n0)
    assert bytes(o0) == p0
    plants = []
    for ch, r in enumerate((py.rl, py.rr)):
        words, idx = np.array(r.mt.mt, dtype=np.uint32), r.mt.i
        if ch == 0:
            off = twists[0] * N + 200 - idx
            off += off & 1
            if W > 2:
                off += 2                            # not the sample's first pair
        else:
            idx |= 1
            off = (twists[1] + 1) * N - 1 - idx
        assert off % 2 == 0
        plants.append((words, idx, off))
    return cfg, nodes, raw, n, st, py, plants


@pytest.mark.parametrize("rtype", [1, 2, 3, 4])
def test_oracle_renders_planted_rejections_as_the_python_restatement(oracle, rtype):
    n0 = 37
    cfg, nodes, raw, n, st, py, plants = _planted_pair(oracle, rtype, n0, (3, 5))
    W = W_OF[rtype]
    for ch, (words, idx, off) in enumerate(plants):
        w = mtplant.plant(words, idx, [off, off + 1])
        rej, _ = mtplant.consumption(w, idx, W, n)
        assert [o for _, o in rej] == [off] and rej[0][0] == off // W, "the pair is not consumed as a pair"
        assert 3 * N <= idx + off < 6 * N           # three to five twists ahead
        st.set_mt(ch, w, idx)
        r = (py.rl, py.rr)[ch]
        r.mt.mt, r.mt.i = [int(v) for v in w], idx
    seg = raw[n0 * 4:]
    out, pre = st.process(seg, n, want_pre=True)
    pout, ppre = py.process(seg, n)
    assert np.array_equal(pre.view(np.uint64), np.array(ppre).view(np.uint64))
    assert bytes(out) == pout
    m = st.meters()
    assert list(m["clips"]) == py.meters["clips"] and list(m["peak_db"]) == py.meters["peak"]


@pytest.mark.parametrize("rtype", [1, 2, 3, 4])
def test_negative_control_one_planted_word_changed(oracle, rtype):
    """with one word of the planted pair set to a value whose tempered >> 5 is not 0, nothing is rejected,
    and the bytes differ from the planted run's from the planted sample on (the walk back changes a few
    words of the generations before it too, so the samples ahead of it are not compared)"""
    n0 = 37
    cfg, nodes, raw, n, st, _, plants = _planted_pair(oracle, rtype, n0, (3, 5))
    st2 = oracle.Stream(cfg, nodes)
    st2.process(raw[:n0 * 4], n0)
    W = W_OF[rtype]
    first = []
    for ch, (words, idx, off) in enumerate(plants):
        w = mtplant.plant(words, idx, [off, off + 1])
        st.set_mt(ch, w, idx)
        # the same generation with one word of the pair made 0x80000000 (tempered: nonzero above bit 6), walked back
        g = (idx + off) // N
        a = w
        for _ in range(g):
            a = mtplant.twist(a)
        a = a.copy()
        p = (idx + off) % N
        assert a[p] == 0
        if p == 623:                                # word 623 is bound to words 396 and 0: change the pair's second
            a[397] ^= 0x80000000                    # word instead, word 0 of the next generation
            assert mtplant.temper(mtplant.twist(a)[:1])[0] >> 6 != 0
        else:
            a[p] = 0x80000000
            assert mtplant.temper(a[p:p + 1])[0] >> 5 != 0
            if p == 0:
                a[623] = a[396] ^ mtplant.f(a[0] & mtplant.LO)
        for _ in range(g):
            a = mtplant.untwist(a)
        rej, _ = mtplant.consumption(a, idx, W, n)
        assert rej == []
        st2.set_mt(ch, a, idx)
        first.append(off // W)
    seg = raw[n0 * 4:]
    o1, _ = st.process(seg, n)
    o2, _ = st2.process(seg, n)
    o1, o2 = o1.reshape(n, 2, 2), o2.reshape(n, 2, 2)
    for ch in range(2):
        t = first[ch]
        # from the planted sample on every draw is another one.  The dither spans 2^1.5 - 1 = 1.8 LSB either
        # way, so two independent draws round to different 16-bit values in well over a quarter of the samples
        frac = np.mean(np.any(o1[t:, ch] != o2[t:, ch], axis=1))
        print(f"render type {rtype} ch {ch}: {frac:.3f} of the samples from {t} on differ")
        assert frac > 0.25
