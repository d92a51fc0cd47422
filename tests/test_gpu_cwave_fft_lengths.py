"""GPU: the direct-FFT CWAVE encoder (icw_encode_cwave_fft, kernel KX `icw_fft_pass`) at every transform length
P = 2^logP, logP 1..24 and 27, at the default cap, and with tracks of equal length in one launch.

test_gpu_cwave_fft.py runs logP 1, 2, 6, 7, 12, 13, 16 and batches of pairwise different logP.  Here:
  (a) dense sweep, logP 1..18, n = 2^logP (the full transform) and 2^(logP-1) + 1 (the shortest track of that P:
      nearly half the tiles lie past the track), random int16 mono; stereo at logP 3, 5, 9, 14, 15.  The check is
      that file's: I bit for bit, Q within cwfft_ref.tolerance of the long-double transform.
  (b) sparse sweep, logP 10, 14, 18, 19..24: 16 impulses, whose Q has a closed form (cwfft_ref.impulse_q) that
      costs O(points checked).  I over the whole track; Q at a probe set against the closed form under
      impulse_tolerance (tolerance's formula, e_np over the probes); Q at every frame against numpy.fft's
      float64 transform under twice that bound: both are float64 transforms held to the bound against the same
      truth, so no tile, column or track offset can be wrong anywhere.  At logP 10, 14, 18 the closed form and the
      long-double transform must give the same verdict.  logP >= 22 goes through device pointers.
  (c) logP 27, n = 2^27 - 37, device pointers: I over the whole track, Q at the probes under the floor term
      2^-52 * 27 * max|reference| alone (numpy.fft at 2^27 points takes far longer than a test may).
  (d) tracks of equal logP in one call (blockIdx.y > 0, the second track's workspace, input, output and clip
      slots): bytes and clip counts equal to the stand-alone encode, host and device pointers, files.
The frames are filled with 0xFF (NaN doubles) before a device-pointer call, so a frame that is never written
fails the comparison.  Fixed seeds.  With ICW_FFT_LENGTHS_RECORD=<path> every accuracy case appends one JSON
line (logP, n, plan, max|err|, e_np, bound, err / bound, reference) to that file.
"""
import json
import os
import struct
import zlib

import numpy as np
import pytest

from in_cwave_amd import abi, synth
from in_cwave_amd import lib as L

import cwenc_ref
import cwfft_ref as R
import wavgen as W

pytestmark = pytest.mark.gpu

LD = np.longdouble
CAP = 7                                                      # ICW_FFT_PASS_LOG2, the default cap
TILE_LOG2 = 11                                               # ICW_FFT_TILE_LOG2


def plan(logP, cap=CAP):
    """icw_fft_plan restated: k = ceil(logP / cap) passes, the stages spread evenly, the longer ones first"""
    k = -(-logP // cap)
    return [logP // k + (1 if i < logP % k else 0) for i in range(k)]


def record(case, logP, n, err, e_np, bound, ref, **more):
    """e_np None: not computed (the bound is the floor term alone)"""
    path = os.environ.get("ICW_FFT_LENGTHS_RECORD")
    print(f"{case} logP {logP} n {n} plan {plan(logP)}: err {err:.3e} e_np {e_np if e_np is None else f'{e_np:.3e}'} "
          f"bound {bound:.3e} err/bound {err / bound if bound else 0.0:.3f} ({ref})")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "logP": logP, "n": n, "plan": plan(logP), "max_err": err, "e_np": e_np,
                                "bound": bound, "err_over_bound": err / bound if bound else 0.0,
                                "err_over_e_np": err / e_np if e_np else None, "reference": ref, **more}) + "\n")


def reference(raw, ch):
    """(x, q, tol) of an int16 track: the unpacked samples, the long-double Q and its tolerance per channel"""
    x = cwenc_ref.unpack(raw, abi.FMT_I16, ch)
    q = [R.hilbert_q(x[:, c]) for c in range(ch)]
    return x, q, [R.tolerance(x[:, c], q[c]) for c in range(ch)]


def check_dense(case, logP, ref, frames):
    """test_gpu_cwave_fft.check_accuracy for one track and its reference()"""
    x, qs, tols = ref
    n, ch = x.shape
    I, Q = cwenc_ref.iq_of_f64_frames(frames, ch)
    assert I.shape == (n, ch)
    assert np.array_equal(I.view(np.uint64), x.view(np.uint64)), f"{case}: I is not the unpacked sample"
    for c in range(ch):
        q = qs[c]
        bound, e_np = tols[c]
        err = float(np.max(np.abs(Q[:, c].astype(LD) - q)))
        record(f"{case} ch {c}", logP, n, err, e_np, bound, "hilbert_q (long-double FFT)")
        assert err <= bound, f"{case} n {n} ch {c}: {err} > {bound} (e_np {e_np})"


# ------------------------------------------------------------------ (a) dense sweep
def _lengths(logP):
    return [2] if logP == 1 else [1 << logP, (1 << (logP - 1)) + 1]


@pytest.mark.parametrize("logP,n", [(lp, n) for lp in range(1, 19) for n in _lengths(lp)])
def test_dense_sweep(icw, logP, n):
    assert R.pad_len(n) == 1 << logP
    assert L.encode_cwave_fft_passes(n, 0) == -(-logP // CAP) == len(plan(logP))
    raw = R.random_pcm16(np.random.default_rng(2000 + n), n, 1)
    (frames,), (clipped,) = L.encode_cwave_fft([raw], abi.FMT_I16, 1)
    assert frames.size == n * 16 and clipped == 0
    check_dense("dense mono", logP, reference(raw, 1), frames)


@pytest.mark.parametrize("logP,n", [(lp, n) for lp in (3, 5, 9, 14, 15) for n in _lengths(lp)])
def test_dense_sweep_stereo(icw, logP, n):
    raw = R.random_pcm16(np.random.default_rng(3000 + n), n, 2)
    (frames,), (clipped,) = L.encode_cwave_fft([raw], abi.FMT_I16, 2)
    assert frames.size == n * 32 and clipped == 0
    check_dense("dense stereo", logP, reference(raw, 2), frames)


# ------------------------------------------------------------------ (b), (c) sparse sweep
K_IMPULSES = 16


def impulses(n, seed):
    """(pos, amp): K_IMPULSES frames with amplitudes in +-30000, among them frame 0, frame n - 1, an odd frame and
    a frame of the last tile; the others wherever the rng puts them"""
    rng = np.random.default_rng(seed)
    tile0 = ((n - 1) >> TILE_LOG2) << TILE_LOG2              # the first frame of the last tile that holds one
    pos = [0, n - 1, 2 * int(rng.integers(0, (n - 1) // 2)) + 1]
    while tile0 < n - 1 and len(pos) < 4:                    # (where frame n - 1 is that tile's only one, it is in)
        p = int(rng.integers(tile0, n - 1))
        if p not in pos:
            pos.append(p)
    while len(pos) < K_IMPULSES:
        p = int(rng.integers(0, n))
        if p not in pos:
            pos.append(p)
    amp = rng.integers(1, 30001, size=K_IMPULSES) * rng.choice([-1, 1], size=K_IMPULSES)
    return np.array(pos, dtype=np.int64), amp.astype(np.float64)


def probes(n, pos, seed):
    """2^15 rng frames, every impulse with its neighbours up to +-2, the first and the last 64 frames"""
    rng = np.random.default_rng(seed)
    near = (pos[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    at = np.concatenate([rng.integers(0, n, size=1 << 15), near, np.arange(min(64, n)), np.arange(max(0, n - 64), n)])
    return np.unique(at[(at >= 0) & (at < n)])


def encode_mono_f64(n, raw16, device):
    """(I, Q) of the CW_F64 frames of one int16 mono track: numpy arrays through host pointers, torch tensors on
    the GPU through device pointers (frames pre-filled with NaN)"""
    if not device:
        (frames,), (clipped,) = L.encode_cwave_fft([raw16.view(np.uint8)], abi.FMT_I16, 1)
        assert frames.size == n * 16 and clipped == 0
        I, Q = cwenc_ref.iq_of_f64_frames(frames, 1)
        return I[:, 0], Q[:, 0]
    import torch
    d_in = raw16 if isinstance(raw16, torch.Tensor) else torch.from_numpy(raw16).cuda()
    d_out = torch.full((n * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    assert L.encode_cwave_fft_device(d_in, [0], [n], abi.FMT_I16, 1, d_out, [0]) == [0]
    iq = d_out.view(torch.float64).view(n, 2)
    return iq[:, 0], iq[:, 1]


SPARSE = [(lp, (1 << lp) - 37) for lp in (10, 14, 18)]
for _lp in range(19, 25):
    SPARSE += [(_lp, (1 << _lp) - 37), (_lp, (1 << (_lp - 1)) + 1)]


@pytest.mark.parametrize("logP,n", SPARSE)
def test_sparse_sweep(icw, logP, n):
    """the whole-length comparison with numpy.fft runs at every length, logP 24 included"""
    assert R.pad_len(n) == 1 << logP and L.encode_cwave_fft_passes(n, 0) == len(plan(logP))
    pos, amp = impulses(n, 4000 + 2 * logP + (n <= 3 << (logP - 2)))
    at = probes(n, pos, 5000 + logP)
    x = R.impulse_track(n, pos, amp)
    raw16 = x.astype("<i2")
    q_cf = R.impulse_q(n, pos, amp, at)
    q_np = R.hilbert_q_np(x)
    bound, e_np = R.impulse_tolerance(n, pos, amp, at, q_cf, q_np=q_np)
    device = logP >= 22
    I, Q = encode_mono_f64(n, raw16, device)
    if device:
        import torch
        # 1. I, whole track, on the device
        assert torch.equal(I.view(torch.int64), torch.from_numpy(x).cuda().view(torch.int64)), "I is not the sample"
        q_at = Q[torch.from_numpy(at).cuda()].cpu().numpy()
        err_all = float((Q - torch.from_numpy(q_np).cuda()).abs().max().cpu())
        del I, Q
    else:
        assert np.array_equal(I.view(np.uint64), x.view(np.uint64)), "I is not the sample"
        q_at = Q[at]
        err_all = float(np.max(np.abs(Q - q_np)))
    # 2. Q at the probes against the closed form
    err = float(np.max(np.abs(q_at.astype(LD) - q_cf)))
    record("sparse, " + ("device" if device else "host") + " pointers", logP, n, err, e_np, bound,
           "impulse_q (closed form) at the probes", probes=int(at.size), whole_track_err_vs_numpy_fft=err_all)
    assert err <= bound, f"logP {logP} n {n}: {err} > {bound} (e_np {e_np})"
    # 3. Q at every frame against numpy.fft: NaN (a frame never written) fails it too
    assert err_all <= 2 * bound, f"logP {logP} n {n}: whole track {err_all} > {2 * bound}"
    if logP <= 18:
        # the long-double transform gives the same verdict as the closed form
        q_ld = R.hilbert_q(x)
        bound_ld, _ = R.tolerance(x, q_ld)
        err_ld = float(np.max(np.abs(Q.astype(LD) - q_ld)))
        print(f"  against hilbert_q: {err_ld:.3e}, bound {bound_ld:.3e}")
        assert (err_ld <= bound_ld) == (err <= bound)


def test_largest_length(icw):
    """logP 27: 2 GiB of workspace and 2 GiB of frames"""
    import torch
    logP = 27
    n = (1 << logP) - 37
    assert L.encode_cwave_fft_passes(n, 0) == 4 and plan(logP) == [7, 7, 7, 6]
    assert L.encode_cwave_fft_workspace([n], 1) >= 16 << logP
    pos, amp = impulses(n, 4027)
    at = probes(n, pos, 5027)
    q_cf = R.impulse_q(n, pos, amp, at)
    bound = 2.0 ** -52 * logP * float(np.max(np.abs(q_cf)))  # the floor term alone
    d_in = torch.zeros(n, dtype=torch.int16, device="cuda")
    d_in[torch.from_numpy(pos).cuda()] = torch.from_numpy(amp.astype(np.int16)).cuda()
    try:
        I, Q = encode_mono_f64(n, d_in, True)
        assert torch.equal(I.view(torch.int64), d_in.to(torch.float64).view(torch.int64)), "I is not the sample"
        assert not bool(torch.isnan(Q).any())                # every frame was written
        q_at = Q[torch.from_numpy(at).cuda()].cpu().numpy()
    finally:
        I = Q = d_in = None
        torch.cuda.empty_cache()
    err = float(np.max(np.abs(q_at.astype(LD) - q_cf)))
    record("largest, device pointers", logP, n, err, None, bound,
           "impulse_q (closed form) at the probes, floor term alone", probes=int(at.size))
    assert err <= bound, f"logP 27: {err} > {bound}"


# ------------------------------------------------------------------ (d) equal lengths in one launch
EQ_N = (3000, 4096, 2049, 3000, 100, 70, 128, 40000, 33000)  # three of logP 12, three of 7 (one pass), two of 16
EQ_LOUD = (0, 4)                                             # full-scale squares in the CW_I16 runs


def _square(n, ch):
    """the `loud` fixture's signal of test_gpu_cwave_fft.py: the Hilbert pair of an edge overshoots int16"""
    k = np.arange(n)
    cols = [np.where((k // (37 + 5 * c)) % 2 == 0, 32767, -32768) for c in range(ch)]
    return np.stack(cols, axis=1).astype("<i2").reshape(-1).view(np.uint8).copy()


@pytest.fixture(scope="module")
def eq_tracks():
    """per channel count and output format the nine tracks' PCM; computed once, never modified.  CW_F64: +-30000
    random, with each track's reference().  CW_I16: +-3000 random (Q stays far inside int16) but for the two
    full-scale squares."""
    assert [R.pad_len(n).bit_length() - 1 for n in EQ_N] == [12, 12, 12, 12, 7, 7, 7, 16, 16]
    res = {}
    for ch in (1, 2):
        res[ch, abi.FMT_CW_F64] = [R.random_pcm16(np.random.default_rng(6000 + 10 * i + ch), n, ch)
                                   for i, n in enumerate(EQ_N)]
        res[ch, abi.FMT_CW_I16] = [
            _square(n, ch) if i in EQ_LOUD else
            np.random.default_rng(7000 + 10 * i + ch).integers(-3000, 3001, size=n * ch).astype("<i2").view(np.uint8).copy()
            for i, n in enumerate(EQ_N)]
        res[ch, "ref"] = [reference(raw, ch) for raw in res[ch, abi.FMT_CW_F64]]
    return res


@pytest.fixture(scope="module")
def eq_alone(icw, eq_tracks):
    """every track encoded alone: (frames, clipped) per track"""
    res = {}
    for (ch, cwf), raws in eq_tracks.items():
        if cwf == "ref":
            continue
        res[ch, cwf] = []
        for raw in raws:
            (f,), (cl,) = L.encode_cwave_fft([raw], abi.FMT_I16, ch, cwf)
            res[ch, cwf].append((f, cl))
    return res


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("cw_format", [abi.FMT_CW_F64, abi.FMT_CW_I16], ids=["f64", "i16"])
@pytest.mark.parametrize("ch", [1, 2])
def test_equal_lengths_in_one_launch(icw, eq_tracks, eq_alone, ch, cw_format, device):
    raws, alone = eq_tracks[ch, cw_format], eq_alone[ch, cw_format]
    fb = L.cwave_frame_bytes(cw_format, ch)
    assert not np.array_equal(raws[0], raws[3])              # the two 3000-frame tracks differ
    if not device:
        together, clips = L.encode_cwave_fft(raws, abi.FMT_I16, ch, cw_format)
    else:
        import torch
        d_in = torch.from_numpy(np.concatenate(raws)).cuda()
        ioff = np.concatenate([[0], np.cumsum([r.size for r in raws])])[:-1]
        ooff, o = [], 3
        for n in EQ_N:                                       # odd offsets, gaps between the tracks
            ooff.append(o)
            o += n * fb + 5
        d_out = torch.zeros(o + 16, dtype=torch.uint8, device="cuda")
        clips = L.encode_cwave_fft_device(d_in, ioff, EQ_N, abi.FMT_I16, ch, d_out, ooff, cw_format)
        got = d_out.cpu().numpy()
        together = [got[b:b + n * fb] for b, n in zip(ooff, EQ_N)]
        covered = np.zeros(got.size, bool)
        for b, n in zip(ooff, EQ_N):
            covered[b:b + n * fb] = True
        assert not got[~covered].any()                       # nothing outside the frames
    for i, n in enumerate(EQ_N):
        assert together[i].size == n * fb
        assert np.array_equal(together[i], alone[i][0]), f"track {i} (n {n}) differs from its stand-alone encode"
        assert clips[i] == alone[i][1], f"track {i} (n {n}): clip count {clips[i]}, alone {alone[i][1]}"
        if cw_format == abi.FMT_CW_I16:
            # a count on a neighbour's slot shows here: the quiet tracks clip nothing, the squares do
            assert (clips[i] > 0) == (i in EQ_LOUD), f"track {i} (n {n}): clip count {clips[i]}"
        else:
            assert clips[i] == 0
            logP = R.pad_len(n).bit_length() - 1
            check_dense(f"equal lengths, {'device' if device else 'host'} pointers, track {i}", logP, eq_tracks[ch, "ref"][i], together[i])


def test_equal_lengths_files(tmp_path, icw):
    """three int16 stereo files of logP 12 at three rates: one group, one launch"""
    specs = [(44100, 3000), (48000, 4096), (96000, 2049)]
    ins, outs, pcm = [], [], []
    for i, (fs, n) in enumerate(specs):
        d = synth.stream_pcm(10 + i, n, fs)
        ins.append(W.write(tmp_path / f"e{i}.wav", d, abi.FMT_I16, 2, fs))
        outs.append(tmp_path / f"e{i}.cwave")
        pcm.append(d)
    rc, st, status, clipped = L.cwave_encode_files_fft(ins, outs)
    assert rc == abi.OK and status == [abi.OK] * 3 and st.n_groups == 1 and st.n_files == 3 and clipped == [0] * 3
    for (fs, n), out, d in zip(specs, outs, pcm):
        img = np.frombuffer(out.read_bytes(), np.uint8)
        magic, hsize, ver, hfmt, hch, hn, hrate, hM, hcrc = struct.unpack("<8s6IiI", img[:40].tobytes())
        assert (magic, hsize, ver, hfmt, hch, hn, hrate, hM) == (b"cPLXwAVE", 48, 2, 0, 2, n, fs, -1)
        data = img[48:]
        (ref,), _ = L.encode_cwave_fft([d], abi.FMT_I16, 2)
        assert np.array_equal(data, ref), out.name
        assert zlib.crc32(data.tobytes()) == hcrc, out.name
