"""Planting rejected dsopen pairs far ahead in an MT19937 stream (test infrastructure).

mtrnd_gen_dsopen (mt_jrnd.c:245-256) rejects a draw of exactly -1.0: a pair of words whose tempered
values are (a, b) with a >> 5 == 0 and b >> 6 == 0.  Tempering is a bijection that maps 0 to 0, so a pair
of zero state words is a rejected pair.  Zeroing words of the *current* state reaches only the next 624
words; a test of the dither generator's chunks needs the pair tens of thousands of words ahead.  The
twist (mt_jrnd.c:105-120) is invertible, so the state k twists ahead can be chosen and walked back:

    new[i] = x ^ f(y),  y = (old[i] & HI) | (old[i + 1] & LO),  f(y) = (y >> 1) ^ (MAG if y & 1)
    x = old[i + 397] for i < 227, new[i - 227] for 227 <= i < 623, and word 623 takes new[0] for old[i + 1]

f's top bit is y & 1 (MAG's top bit is set, y >> 1 has none), so f is undone by invf.  A twist output
carries 623 free words and one bit: word 623 is new[396] ^ f(h | (new[0] & LO)) with h the one free bit,
and old[0]'s low 31 bits are read by nothing, so untwist() sets them so that its result is a twist output
again.

Offsets count words consumed from the call's start: the word at offset o is word (idx + o) mod 624 of
generation (idx + o) // 624, generation 0 being the state itself.  dsopen consumes pairs aligned to the
call's start, and a rejection consumes a whole pair, so the alignment survives it.

consumption() is a small numpy model of what the renders consume (sound_render_value, sound_render.c:711-751:
V = W / 2 dsopen values per sample), independent of the oracle and of the GPU code: which sample takes
each rejected pair, and where a sample's words start.
"""
import numpy as np

HI, LO, MAG = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)
N, M = 624, 397
_ONE = np.uint32(1)


def f(y):
    y = np.asarray(y, dtype=np.uint32)
    return (y >> _ONE) ^ np.where(y & _ONE, MAG, np.uint32(0)).astype(np.uint32)


def invf(z):
    z = np.asarray(z, dtype=np.uint32)
    odd = (z & HI) != 0
    z = np.where(odd, z ^ MAG, z).astype(np.uint32)
    return ((z << _ONE) | odd.astype(np.uint32)).astype(np.uint32)


def temper(y):
    y = np.asarray(y, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def twist(s):
    """the 624-word regeneration, in its three dependency phases and word 623"""
    s = np.asarray(s, dtype=np.uint32)
    new = np.empty(N, dtype=np.uint32)
    y = (s[:-1] & HI) | (s[1:] & LO)                      # y[i] for i < 623
    new[:227] = s[M:] ^ f(y[:227])
    new[227:454] = new[:227] ^ f(y[227:454])
    new[454:623] = new[227:396] ^ f(y[454:623])
    new[623] = new[396] ^ f((s[623] & HI) | (new[0] & LO))
    return new


def untwist(new):
    """the state whose twist is `new` (a twist output), itself a twist output: its word 0 keeps the top bit
    the twist read and takes the low 31 bits that make word 623 consistent"""
    new = np.asarray(new, dtype=np.uint32)
    y = np.empty(N, dtype=np.uint32)
    y[227:] = invf(new[227:] ^ new[:M])                  # x = new[i - 227]
    old = np.empty(N, dtype=np.uint32)
    old[M:] = (y[M:] & HI) | (y[M - 1:N - 1] & LO)       # complete from y[396..623]
    y[:227] = invf(new[:227] ^ old[M:])                  # x = old[i + 397]
    old[1:M] = (y[1:M] & HI) | (y[:M - 1] & LO)
    old[0] = (y[0] & HI) | (invf(old[623] ^ old[396]) & LO)
    return old


def plant(state_words, idx, word_offsets):
    """-> the 624 words to put into the state (with the same idx) so that the words at `word_offsets`,
    counted in words consumed from this state on, are zero.  The offsets must lie in one generation g;
    words i < 226 of generation g + 1 may be asked for as well (word 623 of g with word 0 of g + 1 is the
    pair that straddles a twist).  Every other word of generation g keeps the value the state would have
    reached anyway, but for words 396 / 623 (the twist-output constraint) and i + 397 for each word i asked
    of generation g + 1."""
    s = np.asarray(state_words, dtype=np.uint32).copy()
    assert s.shape == (N,) and 0 <= idx <= N
    pos = sorted({int(idx) + int(o) for o in word_offsets})
    assert pos and pos[0] >= idx
    g = pos[0] // N
    here = [p - g * N for p in pos if p // N == g]
    nxt = [p - (g + 1) * N for p in pos if p // N == g + 1]
    if len(here) + len(nxt) != len(pos) or any(i >= 226 for i in nxt):    # word 226 would need word 623
        raise ValueError("offsets span more than one generation and the head of the next")
    a = s
    for _ in range(g):
        a = twist(a)
    a = a.copy()
    a[here] = 0
    fixed = set(here)
    if g > 0:
        # a must stay a twist output: word 623 = word 396 ^ f(h | low bits of word 0), h = 0 chosen
        t = f(a[0] & LO)
        if 623 in fixed:
            if 396 in fixed and t != 0:
                raise ValueError("words 396 and 623 of one generation cannot both be chosen")
            a[396] = t
            fixed.add(396)
        else:
            a[623] = a[396] ^ t
    for i in nxt:
        if i + M in fixed:
            raise ValueError(f"word {i} of the next generation needs word {i + M}, which is taken")
        a[i + M] = f((a[i] & HI) | (a[i + 1] & LO))
        fixed.add(i + M)
    for _ in range(g):
        a = untwist(a)
    return a


def words_from(state_words, idx, n):
    """the next n tempered words of the stream (genrand_int32, mt_jrnd.c:99-134)"""
    s = np.asarray(state_words, dtype=np.uint32)
    out = np.empty(n, dtype=np.uint32)
    at, i = 0, int(idx)
    while at < n:
        if i >= N:
            s = twist(s)
            i = 0
        k = min(N - i, n - at)
        out[at:at + k] = temper(s[i:i + k])
        at += k
        i += k
    return out


def consumption(state_words, idx, W, n_samples):
    """-> (rejected, starts): `rejected` lists (sample, word offset) of every rejected pair in the order
    consumed, the sample being the one whose draw consumed it; starts[t] is the word offset at which sample
    t's draw begins (n_samples + 1 entries: the last is where the stream stands after them)."""
    V = W // 2
    n_pairs = n_samples * V
    slack = 64
    while True:
        w = words_from(state_words, idx, 2 * (n_pairs + slack))
        rej = ((w[0::2] >> np.uint32(5)) == 0) & ((w[1::2] >> np.uint32(6)) == 0)
        acc = np.flatnonzero(~rej)                        # pair index of each accepted value, in order
        if acc.size > n_pairs:
            break
        slack *= 2
    starts = np.empty(n_samples + 1, dtype=np.int64)
    # a sample starts with the pair after the previous sample's last accepted one (the first at 0): rejected
    # pairs ahead of a value belong to the draw that skips them
    last = acc[V - 1:n_pairs:V][:n_samples]               # pair of each sample's last value
    starts[0] = 0
    starts[1:] = 2 * (last + 1)
    rejected = []
    for p in np.flatnonzero(rej):
        if 2 * p >= starts[-1]:
            break
        t = int(np.searchsorted(starts, 2 * p, side="right")) - 1
        rejected.append((t, int(2 * p)))
    return rejected, starts
