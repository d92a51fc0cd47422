"""Loader for the in-tree HIP library in_cwave_amd/libicw.so and a thin Pythonic wrapper of the
C ABI (include/icw.h).  There is no CPU fallback: if the library or a HIP device is missing the
calls raise."""
import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import abi

LIB_PATH = Path(__file__).resolve().parent / "libicw.so"
# A/B runs only: ICW_LIB=<name> loads in_cwave_amd/<name> (an alternative in-tree build) instead
if os.environ.get("ICW_LIB"):
    LIB_PATH = Path(__file__).resolve().parent / Path(os.environ["ICW_LIB"]).name
_lib = None


class IcwError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise IcwError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        # PyTorch-ROCm bundles its own HIP runtime; when both live in one process (torch tensors as
        # device buffers) torch's must come up first, or its later initialisation finds no GPU.
        try:
            import torch
            torch.cuda.is_available()
        except ImportError:
            pass
        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in abi.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                if os.environ.get("ICW_LIB"):      # an older A/B build may lack newer entry points
                    continue
                raise IcwError(f"{LIB_PATH} does not export {name}")
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _check(rc, what):
    if rc != abi.OK:
        msg = load().icw_strerror(rc).decode()
        raise IcwError(f"{what} failed: {rc} ({msg})")


def _ptr(x):
    """device/host pointer of a numpy array, torch tensor or int"""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    raise TypeError(type(x))


class _HostBuffer:
    """owner of an icw_host_alloc block; freed when the last array view over it goes away"""

    def __init__(self, nbytes):
        p = C.c_void_p()
        _check(load().icw_host_alloc(nbytes, C.byref(p)), "icw_host_alloc")
        self.ptr = p.value

    def __del__(self):
        if self.ptr and _lib is not None:
            _lib.icw_host_free(self.ptr)
            self.ptr = None


class HostArray(np.ndarray):
    """a numpy array over an icw_host_alloc block; the block lives as long as the array or any view"""
    _icw_owner = None


def host_array(shape, dtype=np.uint8):
    """a numpy array in pinned host memory (icw_host_alloc): as a call's in / out buffer its copies
    run block by block beside the kernels"""
    dt = np.dtype(dtype)
    n = max(1, int(np.prod(shape)) * dt.itemsize)
    owner = _HostBuffer(n)
    buf = (C.c_uint8 * n).from_address(owner.ptr)
    a = np.frombuffer(buf, dtype=np.uint8, count=int(np.prod(shape)) * dt.itemsize).view(dt).reshape(shape)
    a = a.view(HostArray)
    a._icw_owner = owner
    return a


class Context:
    """One icw_ctx: n_streams streams sharing a config and a DSP list, state resident in HBM."""

    def __init__(self, cfg, nodes, n_streams, device=-1):
        lib = load()
        self._lib = lib
        arr = (abi.Node * max(1, len(nodes)))(*nodes) if nodes else (abi.Node * 1)()
        h = C.c_void_p()
        acc = C.c_int()
        _check(lib.icw_create(C.byref(cfg), arr, len(nodes), n_streams, device, C.byref(h), C.byref(acc)),
               "icw_create")
        self.h = h
        self.accepted = bool(acc.value)
        self.cfg = cfg
        self.n_streams = n_streams
        self.render_size = lib.icw_render_size(h)
        self.stream_rs = [self.render_size] * n_streams   # every stream's own sample bytes (set_stream_render)
        self.fsz = abi.FMT_BYTES[cfg.in_format] * cfg.in_channels
        self.stream_fsz = [self.fsz] * n_streams       # every stream's own frame bytes (set_stream_input)
        self.stream_channels = [int(cfg.in_channels)] * n_streams   # and channels (the encoders' frame bytes)

    def close(self):
        if self.h:
            self._lib.icw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream_init(self, first=0, count=None):
        _check(self._lib.icw_stream_init(self.h, first, self.n_streams - first if count is None else count),
               "icw_stream_init")

    def set_input(self, sample_rate, fmt, channels):
        """a new track's sample format for every stream (icw_set_input)"""
        _check(self._lib.icw_set_input(self.h, sample_rate, fmt, channels), "icw_set_input")
        self.fsz = abi.FMT_BYTES[fmt] * channels
        self.stream_fsz = [self.fsz] * self.n_streams
        self.stream_channels = [int(channels)] * self.n_streams

    def set_stream_input(self, sample_rate, fmt, channels, first=0, count=None):
        """icw_set_stream_input: the input of streams [first, first + count) for the next calls.  A call's
        rows then hold each stream's frames at its own frame size (stream_fsz), in rows as wide as the
        call's widest stream needs.  fsz is the streams' common frame size: while they differ it keeps its
        last value, and the helpers size their rows by call_fsz()."""
        count = self.n_streams - first if count is None else count
        _check(self._lib.icw_set_stream_input(self.h, int(first), int(count), sample_rate, fmt, channels),
               "icw_set_stream_input")
        self.stream_fsz[first:first + count] = [abi.FMT_BYTES[fmt] * channels] * count
        self.stream_channels[first:first + count] = [int(channels)] * count
        if len(set(self.stream_fsz)) == 1:
            self.fsz = self.stream_fsz[0]

    def stream_input_count(self):
        """icw_stream_input_count: distinct inputs in force (1 on a fresh context)"""
        return int(self._lib.icw_stream_input_count(self.h))

    def call_fsz(self, first=0, count=None):
        """the widest frame among streams [first, first + count): what a call's input rows are sized by"""
        count = self.n_streams - first if count is None else count
        return max(self.stream_fsz[first:first + count])

    def set_fir_hilbert(self, order, beta=8.0):
        """icw_set_fir_hilbert: real input through the FIR Hilbert converter (order k_M, Kaiser
        beta k_beta, cwave.h:56-58) instead of the quadrature IIR; order 0 restores the IIR"""
        _check(self._lib.icw_set_fir_hilbert(self.h, order, beta), "icw_set_fir_hilbert")

    def enable_stream_fir(self, on=True):
        """icw_enable_stream_fir: per-stream lists and inputs beside the FIR converter (off on a fresh context)"""
        _check(self._lib.icw_enable_stream_fir(self.h, int(bool(on))), "icw_enable_stream_fir")

    def set_stream_fir(self, order, beta=8.0, first=0, count=None):
        """icw_set_stream_fir: the FIR Hilbert converter (order k_M, Kaiser beta) of streams [first, first + count)
        for the next calls; their FIR history restarts, the other streams keep theirs"""
        count = self.n_streams - first if count is None else count
        _check(self._lib.icw_set_stream_fir(self.h, int(first), int(count), int(order), float(beta)), "icw_set_stream_fir")

    def stream_fir_count(self):
        """icw_stream_fir_count: distinct (k_M, k_beta) in force (1 on a fresh context and with the converter off)"""
        return int(self._lib.icw_stream_fir_count(self.h))

    def enable_stream_bus(self, on=True):
        """icw_enable_stream_bus: set_stream_graph takes bus-form lists (feedback, delays, more than 16 nodes),
        each stream with its own, and set_graph takes one while the lists differ (off on a fresh context)"""
        _check(self._lib.icw_enable_stream_bus(self.h, int(bool(on))), "icw_enable_stream_bus")

    def enable_stream_encode(self, on=True):
        """icw_enable_stream_encode: the CWAVE encoders serve streams with different inputs (off on a fresh
        context)"""
        _check(self._lib.icw_enable_stream_encode(self.h, int(bool(on))), "icw_enable_stream_encode")

    def enable_stream_cwave(self, on=True):
        """icw_enable_stream_cwave: set_stream_input takes the CWAVE formats, also on a context whose input is
        CWAVE (off on a fresh context); a call then covers streams of one kind"""
        _check(self._lib.icw_enable_stream_cwave(self.h, int(bool(on))), "icw_enable_stream_cwave")

    def encode_frame_bytes(self, cw_format, first=0, count=None):
        """every stream's own CWAVE frame bytes in [first, first + count): an encode call's output rows hold
        stream i's frames at this size, in rows as wide as the call's widest stream needs"""
        count = self.n_streams - first if count is None else count
        return [cwave_frame_bytes(cw_format, ch) for ch in self.stream_channels[first:first + count]]

    def _own_cfg(self):
        """the live setters record the context's parameters in a copy, never in the caller's Config"""
        self.cfg = abi.Config.from_buffer_copy(self.cfg)

    def set_graph(self, nodes, bypass_list=0):
        """live DSP-list edit for the next calls (icw_set_graph); returns False when the list is
        one amod_init would reject (the running list stays)"""
        arr = (abi.Node * max(1, len(nodes)))(*nodes) if nodes else (abi.Node * 1)()
        acc = C.c_int()
        rc = self._lib.icw_set_graph(self.h, arr, len(nodes), int(bypass_list), C.byref(acc))
        if rc == abi.EGRAPH:
            return False
        _check(rc, "icw_set_graph")
        self._own_cfg()
        self.cfg.bypass_list = int(bool(bypass_list))
        return True

    def clear_bus_slot(self, slot):
        """mod_context_clear_all_inouts for every stream (icw_clear_bus_slot): slot 0..26 to zero"""
        _check(self._lib.icw_clear_bus_slot(self.h, int(slot)), "icw_clear_bus_slot")

    def set_stream_graph(self, nodes, first=0, count=None, bypass_list=0):
        """icw_set_stream_graph: the DSP list of streams [first, first + count) for the next calls;
        returns False when the list is one amod_init would reject (the running lists stay)"""
        count = self.n_streams - first if count is None else count
        arr = (abi.Node * max(1, len(nodes)))(*nodes) if nodes else (abi.Node * 1)()
        acc = C.c_int()
        rc = self._lib.icw_set_stream_graph(self.h, int(first), int(count), arr, len(nodes), int(bypass_list),
                                            C.byref(acc))
        if rc == abi.EGRAPH:
            return False
        _check(rc, "icw_set_stream_graph")
        return True

    def clear_stream_bus_slot(self, slot, first=0, count=None):
        """icw_clear_stream_bus_slot: bus slot 0..26 of streams [first, first + count) to zero"""
        count = self.n_streams - first if count is None else count
        _check(self._lib.icw_clear_stream_bus_slot(self.h, int(first), int(count), int(slot)),
               "icw_clear_stream_bus_slot")

    def stream_graph_count(self):
        """icw_stream_graph_count: distinct compiled lists in force (1 on a fresh context)"""
        return int(self._lib.icw_stream_graph_count(self.h))

    def graph_del_last(self):
        """amod_del_lastdsp (icw_graph_del_last): the tail goes, its output slot is cleared"""
        _check(self._lib.icw_graph_del_last(self.h), "icw_graph_del_last")

    def graph_del_all(self):
        """amod_del_dsplist (icw_graph_del_all): every node but the Master, each slot cleared"""
        _check(self._lib.icw_graph_del_all(self.h), "icw_graph_del_all")

    def graph_add_last(self, node):
        """amod_add_lastdsp + the GUI's field writes (icw_graph_add_last); False if refused"""
        rc = self._lib.icw_graph_add_last(self.h, C.byref(node))
        if rc == abi.EGRAPH:
            return False
        _check(rc, "icw_graph_add_last")
        return True

    def graph_set_output_plug(self, index, n):
        """amod_set_output_plug (icw_graph_set_output_plug): node `index`'s slot to n (-1: clear only)"""
        _check(self._lib.icw_graph_set_output_plug(self.h, int(index), int(n)), "icw_graph_set_output_plug")

    def prepare(self, n_frames=0):
        """icw_prepare: warm a fresh context (one call of silence, then the fresh state back)"""
        _check(self._lib.icw_prepare(self.h, int(n_frames)), "icw_prepare")

    def set_render(self, render):
        """srenders_set_vcfg for every stream (icw_set_render): an abi.RenderCfg"""
        _check(self._lib.icw_set_render(self.h, C.byref(render)), "icw_set_render")
        self._own_cfg()
        self.cfg.render = render

    def set_outbits(self, need24bits):
        """sound_render_set_outbits for every stream (icw_set_outbits): 16 or 24 output bits"""
        _check(self._lib.icw_set_outbits(self.h, int(bool(need24bits))), "icw_set_outbits")
        self._own_cfg()
        self.cfg.need24bits = int(bool(need24bits))
        self.render_size = self._lib.icw_render_size(self.h)
        self.stream_rs = [self.render_size] * self.n_streams

    def set_stream_render(self, render, need24bits, first=0, count=None):
        """icw_set_stream_render: the render (an abi.RenderCfg) and the output depth of streams
        [first, first + count) for the next calls.  A call's output rows then hold each stream's frames at
        its own size (2 * stream_render_size(s)), in rows as wide as the call's widest stream needs;
        render_size is the largest in force."""
        count = self.n_streams - first if count is None else count
        _check(self._lib.icw_set_stream_render(self.h, int(first), int(count), C.byref(render), int(bool(need24bits))),
               "icw_set_stream_render")
        self.stream_rs[first:first + count] = [3 if need24bits else 2] * count
        self.render_size = self._lib.icw_render_size(self.h)

    def stream_render_count(self):
        """icw_stream_render_count: distinct (render, depth) pairs in force (1 on a fresh context)"""
        return int(self._lib.icw_stream_render_count(self.h))

    def stream_render_size(self, s):
        """icw_stream_render_size: bytes per output channel-sample of stream s, 2 or 3"""
        return int(self._lib.icw_stream_render_size(self.h, int(s)))

    def call_osz(self, first=0, count=None):
        """the widest output frame among streams [first, first + count): what a call's output rows are sized by"""
        count = self.n_streams - first if count is None else count
        return 2 * max(self.stream_rs[first:first + count])

    def set_hilbert_filter(self, type_):
        """mod_context_change_all_hilberts_filter (icw_set_hilbert_filter)"""
        _check(self._lib.icw_set_hilbert_filter(self.h, type_), "icw_set_hilbert_filter")
        self._own_cfg()
        self.cfg.hilbert_type = type_

    def set_hilbert_config(self, kahan, subnorm_reject):
        """mod_context_change_all_hilberts_config (icw_set_hilbert_config)"""
        _check(self._lib.icw_set_hilbert_config(self.h, int(kahan), int(subnorm_reject)), "icw_set_hilbert_config")
        self._own_cfg()
        self.cfg.iir_kahan, self.cfg.iir_subnorm_reject = int(bool(kahan)), int(bool(subnorm_reject))

    def set_stream_hilbert(self, type_, kahan, subnorm_reject, first=0, count=None):
        """icw_set_stream_hilbert: the Hilbert converter (type 0..5, Kahan or baseline summation, the
        subnormal reject) of streams [first, first + count) for the next calls.  cfg is not followed: it
        keeps what the context-wide setters last gave."""
        count = self.n_streams - first if count is None else count
        _check(self._lib.icw_set_stream_hilbert(self.h, int(first), int(count), int(type_), int(bool(kahan)),
                                                int(bool(subnorm_reject))), "icw_set_stream_hilbert")

    def stream_hilbert_count(self):
        """icw_stream_hilbert_count: distinct (type, kahan, reject) settings in force (1 on a fresh context)"""
        return int(self._lib.icw_stream_hilbert_count(self.h))

    def stream_open(self, s, n_samples, fade_in_ms=0, fade_out_ms=0, sec_align=0, clr_nframe=0, clr_hilb=0):
        _check(self._lib.icw_stream_open(self.h, s, n_samples, fade_in_ms, fade_out_ms, sec_align,
                                         clr_nframe, clr_hilb), "icw_stream_open")

    def stream_reset_framecnt(self, s):
        """mod_context_reset_framecnt (icw_stream_reset_framecnt): stream s's modulator frame counter to 0"""
        _check(self._lib.icw_stream_reset_framecnt(self.h, int(s)), "icw_stream_reset_framecnt")

    def process(self, inp, n_frames, first=0, count=None, want_pre=False, out=None):
        """Host numpy path: inp uint8 [count, >= n_frames*fsz]; returns (out uint8 [count, n_frames*2*rs],
        pre float64 [count, n_frames, 2] or None).  out: a preallocated output array (reused).  Streams with
        different renders (set_stream_render): rs is the call's widest, and stream i's frames fill the first
        n_frames * 2 * stream_rs[first + i] bytes of its row."""
        count = self.n_streams - first if count is None else count
        inp = np.ascontiguousarray(inp)
        assert inp.dtype == np.uint8 and inp.shape[0] == count and inp.shape[1] >= n_frames * self.call_fsz(first, count)
        osz = self.call_osz(first, count)       # the widest stream of the call (set_stream_render)
        if out is None:
            out = np.zeros((count, n_frames * osz), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.shape[0] == count
        assert out.shape[1] >= n_frames * osz
        pre = np.zeros((count, n_frames, 2), dtype=np.float64) if want_pre else None
        flags = abi.F_DEBUG_PRE if want_pre else 0
        # a length-1 leading axis may carry stride 0 (x[None, :]): the row length is the stride then
        in_stride = inp.strides[0] if count > 1 else inp.shape[1]
        _check(self._lib.icw_process_streams(self.h, first, count, _ptr(inp), in_stride, _ptr(out),
                                             out.strides[0], n_frames, flags, _ptr(pre), None),
               "icw_process_streams")
        return out, pre

    def unpacked_input(self, inp, n_frames, first=0, count=None):
        """Test hook (ICW_F_DEBUG_INPUT): process like `process` and return float64 [count, n_frames, 2],
        the unpacked, faded samples K0 hands the Hilbert converters (pre-Hilbert, R = L for mono)"""
        count = self.n_streams - first if count is None else count
        inp = np.ascontiguousarray(inp)
        assert inp.dtype == np.uint8 and inp.shape[0] == count and inp.shape[1] >= n_frames * self.call_fsz(first, count)
        out = np.zeros((count, n_frames * 2 * self.render_size), dtype=np.uint8)
        x = np.zeros((count, n_frames, 2), dtype=np.float64)
        in_stride = inp.strides[0] if count > 1 else inp.shape[1]
        _check(self._lib.icw_process_streams(self.h, first, count, _ptr(inp), in_stride, _ptr(out), out.strides[0],
                                             n_frames, abi.F_DEBUG_INPUT, _ptr(x), None), "icw_process_streams")
        return x, out

    def process_device(self, d_in, in_stride, d_out, out_stride, n_frames, first=0, count=None,
                       timing=False, hip_stream=None):
        count = self.n_streams - first if count is None else count
        flags = abi.F_DEVICE_PTRS | (abi.F_TIMING if timing else 0)
        _check(self._lib.icw_process_streams(self.h, first, count, _ptr(d_in), in_stride, _ptr(d_out),
                                             out_stride, n_frames, flags, None, hip_stream),
               "icw_process_streams")

    def encode_cwave(self, inp, n_frames, cw_format=abi.FMT_CW_F64, first=0, count=None, out=None):
        """icw_encode_cwave, host path: inp uint8 [count, >= n_frames*fsz] through the FIR Hilbert converter
        (set_fir_hilbert) to packed CWAVE frames, uint8 [count, n_frames * frame bytes].  Advances the
        converter's history and the reader position like a process call; nothing else.  Streams with different
        inputs (enable_stream_encode): rows at each stream's own frame size in, and out at its own
        encode_frame_bytes, in rows of the call's widest."""
        count = self.n_streams - first if count is None else count
        inp = np.ascontiguousarray(inp)
        assert inp.dtype == np.uint8 and inp.shape[0] == count and inp.shape[1] >= n_frames * self.call_fsz(first, count)
        fb = max(self.encode_frame_bytes(cw_format, first, count))
        if out is None:
            out = np.zeros((count, n_frames * fb), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.shape[0] == count and out.shape[1] >= n_frames * fb
        in_stride = inp.strides[0] if count > 1 else inp.shape[1]
        out_stride = out.strides[0] if count > 1 else out.shape[1]
        _check(self._lib.icw_encode_cwave(self.h, first, count, _ptr(inp), in_stride, _ptr(out), out_stride,
                                          n_frames, cw_format, 0, None), "icw_encode_cwave")
        return out

    def encode_cwave_device(self, d_in, in_stride, d_out, out_stride, n_frames, cw_format=abi.FMT_CW_F64,
                            first=0, count=None, hip_stream=None):
        """icw_encode_cwave with ICW_F_DEVICE_PTRS (torch tensors / int pointers), stream-ordered"""
        count = self.n_streams - first if count is None else count
        _check(self._lib.icw_encode_cwave(self.h, first, count, _ptr(d_in), in_stride, _ptr(d_out), out_stride,
                                          n_frames, cw_format, abi.F_DEVICE_PTRS, hip_stream), "icw_encode_cwave")

    def encode_cwave_iir(self, inp, n_frames, cw_format=abi.FMT_CW_F64, first=0, count=None, out=None):
        """icw_encode_cwave_iir, host path: inp uint8 [count, >= n_frames*fsz] through the context's quadrature
        IIR converter to packed CWAVE frames, uint8 [count, n_frames * frame bytes].  Advances the converters
        (rings, phases, de-subnorm counters) and the reader position like a process call; nothing else.
        Streams with different inputs: as encode_cwave."""
        count = self.n_streams - first if count is None else count
        inp = np.ascontiguousarray(inp)
        assert inp.dtype == np.uint8 and inp.shape[0] == count and inp.shape[1] >= n_frames * self.call_fsz(first, count)
        fb = max(self.encode_frame_bytes(cw_format, first, count))
        if out is None:
            out = np.zeros((count, n_frames * fb), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.shape[0] == count and out.shape[1] >= n_frames * fb
        in_stride = inp.strides[0] if count > 1 else inp.shape[1]
        out_stride = out.strides[0] if count > 1 else out.shape[1]
        _check(self._lib.icw_encode_cwave_iir(self.h, first, count, _ptr(inp), in_stride, _ptr(out), out_stride,
                                              n_frames, cw_format, 0, None), "icw_encode_cwave_iir")
        return out

    def encode_cwave_iir_device(self, d_in, in_stride, d_out, out_stride, n_frames, cw_format=abi.FMT_CW_F64,
                                first=0, count=None, hip_stream=None):
        """icw_encode_cwave_iir with ICW_F_DEVICE_PTRS (torch tensors / int pointers), stream-ordered"""
        count = self.n_streams - first if count is None else count
        _check(self._lib.icw_encode_cwave_iir(self.h, first, count, _ptr(d_in), in_stride, _ptr(d_out), out_stride,
                                              n_frames, cw_format, abi.F_DEVICE_PTRS, hip_stream),
               "icw_encode_cwave_iir")

    def encode_clipped(self, s, reset=False):
        """icw_encode_clipped: saturated / NaN int16 samples stream s has encoded since the last reset"""
        v = C.c_uint64()
        _check(self._lib.icw_encode_clipped(self.h, s, 1 if reset else 0, C.byref(v)), "icw_encode_clipped")
        return v.value

    def synchronize(self):
        _check(self._lib.icw_synchronize(self.h), "icw_synchronize")

    def meters(self, s, reset=False):
        m = abi.Meters()
        _check(self._lib.icw_get_meters(self.h, s, 1 if reset else 0, C.byref(m)), "icw_get_meters")
        return {"clips": (m.clips[0], m.clips[1]), "peak_db": (m.peak_db[0], m.peak_db[1]),
                "desubnorm": m.desubnorm}

    def n_frame(self, s):
        v = C.c_uint64()
        _check(self._lib.icw_n_frame(self.h, s, C.byref(v)), "icw_n_frame")
        return v.value

    def get_state(self, s):
        n = self._lib.icw_state_size(self.h)
        buf = (C.c_uint8 * n)()
        _check(self._lib.icw_get_state(self.h, s, buf, n), "icw_get_state")
        return bytes(buf)

    def set_state(self, s, blob):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        _check(self._lib.icw_set_state(self.h, s, buf, len(blob)), "icw_set_state")

    def fp_census(self, s, reset=False):
        """icw_get_fp_census: uint32 [4, 7] (Hilbert L, R, render L, R) x (total, snan, qnan, ninf,
        nden, pden, pinf)"""
        buf = (C.c_uint32 * (4 * abi.FES_N))()
        _check(self._lib.icw_get_fp_census(self.h, s, 1 if reset else 0, buf), "icw_get_fp_census")
        return np.frombuffer(bytes(buf), dtype=np.uint32).reshape(4, abi.FES_N).copy()

    def last_k1_kernel(self):
        """ICW_K1_* of the last real-input call: 0 lane-per-chain, 1 pair, 2 MFMA, 3 row broadcast"""
        return int(self._lib.icw_last_k1_kernel(self.h))

    def last_dither_chunks(self):
        """icw_last_dither_chunks: (chunks, chunk_frames) of the dither generator over the first launch block of
        the last process call; (0, 0) if that call ran no generator"""
        v = C.c_int()
        n = int(self._lib.icw_last_dither_chunks(self.h, C.byref(v)))
        if n < 0:
            _check(n, "icw_last_dither_chunks")
        return n, v.value

    def last_k0_ms(self):
        """icw_last_k0_timing: K0's time in the last timed call, summed over its launch blocks"""
        v = C.c_double()
        _check(self._lib.icw_last_k0_timing(self.h, C.byref(v)), "icw_last_k0_timing")
        return v.value

    def last_timing(self):
        ms = (C.c_double * 2)()
        n = (C.c_int * 2)()
        _check(self._lib.icw_last_timing(self.h, ms, n), "icw_last_timing")
        return (ms[0], ms[1]), (n[0], n[1])


def fir_taps(order, beta=8.0):
    """icw_fir_taps: the converter's taps g_m, m = 1, 3, .. (host arithmetic, no device call)"""
    g = np.zeros((order // 2 + 1) // 2, dtype=np.float64)
    nt = load().icw_fir_taps(order, beta, _ptr(g), g.size)
    if nt < 0:
        _check(nt, "icw_fir_taps")
    return g


# ------------------------------------------------------------------ CWAVE files / CRC-32 -------
def cwave_parse(header, file_size):
    """icw_cwave_parse: the reference's CWAVE header checks (xwave_reader.c:243-300).  Returns
    (header struct, ICW_FMT_CW_* format, frame bytes); raises IcwError for a refused file."""
    lib = load()
    b = np.frombuffer(bytes(header[:abi.CWAVE_HEADER_BYTES]), dtype=np.uint8).copy()
    h = abi.CwaveHeader()
    fmt, fb = C.c_uint32(), C.c_uint32()
    _check(lib.icw_cwave_parse(_ptr(b), b.size, file_size, C.byref(h), C.byref(fmt), C.byref(fb)), "icw_cwave_parse")
    return h, fmt.value, fb.value


def crc32_batch(base, offsets, lengths, crc_in=None, device_ptrs=False, device=-1, hip_stream=None):
    """icw_crc32_batch: CRC-32 (crc32.c) of the byte ranges [base+offsets[i], +lengths[i]) on the
    GPU.  base: numpy uint8 array (host) or a torch uint8 CUDA tensor / int pointer (device_ptrs)."""
    lib = load()
    n = len(offsets)
    off = (C.c_uint64 * max(1, n))(*[int(v) for v in offsets])
    ln = (C.c_uint64 * max(1, n))(*[int(v) for v in lengths])
    cin = (C.c_uint32 * max(1, n))(*[int(v) for v in crc_in]) if crc_in is not None else None
    out = (C.c_uint32 * max(1, n))()
    flags = abi.F_DEVICE_PTRS if device_ptrs else 0
    _check(lib.icw_crc32_batch(_ptr(base), off, ln, n, cin, out, flags, device, hip_stream), "icw_crc32_batch")
    return [int(out[i]) for i in range(n)]


def crc32_combine(crc_a, crc_b, len_b):
    return int(load().icw_crc32_combine(crc_a, crc_b, len_b))


def cwave_check(image, device_ptrs=False, device=-1, size=None):
    """icw_cwave_check: (crc, ok) with ok 1 / 0, or -1 for a V1 file without a stored CRC"""
    lib = load()
    size = image.numel() if hasattr(image, "numel") else (len(image) if size is None else size)
    crc, ok = C.c_uint32(), C.c_int()
    _check(lib.icw_cwave_check(_ptr(image), size, abi.F_DEVICE_PTRS if device_ptrs else 0, device,
                               C.byref(crc), C.byref(ok)), "icw_cwave_check")
    return crc.value, ok.value


# ------------------------------------------------------------------ in_cwave.cfg ingestion -----
def config_load(text, sample_rate=48000, fmt=abi.FMT_I16, channels=2):
    """icw_config_load on the text of an in_cwave.cfg (load_config, config.c:813-915).
    Returns (ok, FileConfig, bad_line); on failure the FileConfig holds the defaults, as the
    reference falls back to them."""
    data = text.encode() if isinstance(text, str) else bytes(text)
    fc = abi.FileConfig()
    fc.cfg.sample_rate, fc.cfg.in_format, fc.cfg.in_channels = sample_rate, fmt, channels
    bad = C.c_int()
    rc = load().icw_config_load(data, len(data), C.byref(fc), C.byref(bad))
    return rc == abi.OK, fc, bad.value


def config_nodes(fc):
    """the DSP list of a loaded config, head first, as icw_create takes it"""
    return [fc.nodes[i] for i in range(fc.n_nodes)]


def node_dsp_parse(args):
    n = abi.Node()
    name = C.create_string_buffer(abi.DSP_NAME_SIZE)
    _check(load().icw_node_dsp_parse(args.encode() if isinstance(args, str) else args, C.byref(n), name,
                                     abi.DSP_NAME_SIZE), "icw_node_dsp_parse")
    return n, name.value.decode(errors="replace")


def node_dsp_format(node, name=""):
    buf = C.create_string_buffer(4096)
    k = load().icw_node_dsp_format(C.byref(node), name.encode(), buf, 4096)
    if k < 0:
        _check(k, "icw_node_dsp_format")
    return buf.value.decode()


# ------------------------------------------------------------------ WAV / CWAVE files ---------
def wav_parse_file(path):
    """icw_wav_parse_file: the reference's reader acceptance (xwave_reader_create); raises for a
    refused file"""
    info = abi.WavInfo()
    _check(load().icw_wav_parse_file(str(path).encode(), C.byref(info)), "icw_wav_parse_file")
    return info


def _batch_flags(merge_inputs, merge_cwave, merge_bus=False):
    """icw_batch_opts.reserved_: the ICW_BATCH_* bits"""
    return ((abi.BATCH_MERGE_INPUTS if merge_inputs else 0) | (abi.BATCH_MERGE_CWAVE if merge_cwave else 0) |
            (abi.BATCH_MERGE_BUS if merge_bus else 0))


def transcode_files(cfg, nodes, in_paths, out_paths, fade_in_ms=0, fade_out_ms=0, sec_align=0,
                    block_frames=0, device=-1, merge_inputs=False, merge_cwave=False):
    """icw_transcode_files: many files through the GPU path; returns (stats, per-file status).
    merge_inputs: ICW_BATCH_MERGE_INPUTS, all real-input files in one context; merge_cwave:
    ICW_BATCH_MERGE_CWAVE, all CWAVE files in one (another) context"""
    n = len(in_paths)
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    arr = graph_nodes(nodes)
    o = abi.BatchOpts(fade_in_ms, fade_out_ms, sec_align, block_frames, device,
                      _batch_flags(merge_inputs, merge_cwave))
    st = abi.BatchStats()
    status = (C.c_int * max(1, n))()
    rc = load().icw_transcode_files(C.byref(cfg), arr, len(nodes), ins, outs, n, C.byref(o), C.byref(st), status)
    return rc, st, [status[i] for i in range(n)]


def graph_form(cfg, nodes, bypass_list=0):
    """icw_graph_form (host only): 0 register form, 1 bus form, abi.EGRAPH a rejected list"""
    return int(load().icw_graph_form(C.byref(cfg), graph_nodes(nodes), len(nodes), int(bypass_list)))


def transcode_files_lists(cfg, node_lists, in_paths, out_paths, bypass_lists=None, fade_in_ms=0, fade_out_ms=0,
                          sec_align=0, block_frames=0, device=-1, merge_inputs=False, merge_cwave=False, merge_bus=False):
    """icw_transcode_files_lists: file i through its own list node_lists[i] (bypass_lists[i] where
    given); returns (rc, stats, per-file status).  merge_bus: ICW_BATCH_MERGE_BUS, a group's bus-form files in
    one context"""
    n = len(in_paths)
    assert len(node_lists) == n and len(out_paths) == n and (bypass_lists is None or len(bypass_lists) == n)
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    arrs = [graph_nodes(nl) for nl in node_lists]
    ptrs = (C.POINTER(abi.Node) * max(1, n))(*[C.cast(a, C.POINTER(abi.Node)) for a in arrs])
    cnt = (C.c_int * max(1, n))(*[len(nl) for nl in node_lists])
    byp = (C.c_int * max(1, n))(*[int(b) for b in bypass_lists]) if bypass_lists is not None else None
    o = abi.BatchOpts(fade_in_ms, fade_out_ms, sec_align, block_frames, device,
                      _batch_flags(merge_inputs, merge_cwave, merge_bus))
    st = abi.BatchStats()
    status = (C.c_int * max(1, n))()
    rc = load().icw_transcode_files_lists(C.byref(cfg), ptrs, cnt, byp, ins, outs, n, C.byref(o), C.byref(st), status)
    return rc, st, [status[i] for i in range(n)]


def transcode_files_fir(cfg, node_lists, in_paths, out_paths, k_M, k_beta=8.0, bypass_lists=None, fade_in_ms=0,
                        fade_out_ms=0, sec_align=0, block_frames=0, device=-1, merge_inputs=False, merge_cwave=False):
    """icw_transcode_files_fir: transcode_files_lists with the FIR Hilbert converter (k_M, k_beta) on every
    context of real-input files; returns (rc, stats, per-file status)"""
    n = len(in_paths)
    assert len(node_lists) == n and len(out_paths) == n and (bypass_lists is None or len(bypass_lists) == n)
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    arrs = [graph_nodes(nl) for nl in node_lists]
    ptrs = (C.POINTER(abi.Node) * max(1, n))(*[C.cast(a, C.POINTER(abi.Node)) for a in arrs])
    cnt = (C.c_int * max(1, n))(*[len(nl) for nl in node_lists])
    byp = (C.c_int * max(1, n))(*[int(b) for b in bypass_lists]) if bypass_lists is not None else None
    o = abi.BatchOpts(fade_in_ms, fade_out_ms, sec_align, block_frames, device,
                      _batch_flags(merge_inputs, merge_cwave))
    st = abi.BatchStats()
    status = (C.c_int * max(1, n))()
    rc = load().icw_transcode_files_fir(C.byref(cfg), ptrs, cnt, byp, ins, outs, n, int(k_M), float(k_beta), C.byref(o),
                                        C.byref(st), status)
    return rc, st, [status[i] for i in range(n)]


def pool_plan(totals, slots, block_frames=0, order=abi.POOL_AS_GIVEN):
    """icw_pool_plan (host only): the plan icw_transcode_files_pool executes for one pool of files of `totals`
    frames (tails included); returns (rc, per-file slots, per-file start blocks, stats) -- slot and start are -1
    for a file without frames"""
    n = len(totals)
    tot = (C.c_int64 * max(1, n))(*[int(t) for t in totals])
    slot = (C.c_int32 * max(1, n))()
    start = (C.c_int64 * max(1, n))()
    st = abi.PoolStats()
    rc = load().icw_pool_plan(tot, n, int(slots), int(block_frames), int(order), slot, start, C.byref(st))
    return rc, [slot[i] for i in range(n)], [start[i] for i in range(n)], st


def transcode_files_pool(cfg, node_lists, in_paths, out_paths, slots=0, order=abi.POOL_AS_GIVEN, bypass_lists=None,
                         fade_in_ms=0, fade_out_ms=0, sec_align=0, block_frames=0, device=-1, want_meters=True):
    """icw_transcode_files_pool: transcode_files_lists through pools of `slots` streams, a slot refilled with the
    next file of the queue as its file ends; returns (rc, pool stats, per-file status, per-file meters as
    Context.meters gives them -- None with want_meters False)"""
    n = len(in_paths)
    assert len(node_lists) == n and len(out_paths) == n and (bypass_lists is None or len(bypass_lists) == n)
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    arrs = [graph_nodes(nl) for nl in node_lists]
    ptrs = (C.POINTER(abi.Node) * max(1, n))(*[C.cast(a, C.POINTER(abi.Node)) for a in arrs])
    cnt = (C.c_int * max(1, n))(*[len(nl) for nl in node_lists])
    byp = (C.c_int * max(1, n))(*[int(b) for b in bypass_lists]) if bypass_lists is not None else None
    o = abi.PoolOpts(abi.BatchOpts(fade_in_ms, fade_out_ms, sec_align, block_frames, device, 0), int(slots), int(order))
    st = abi.PoolStats()
    status = (C.c_int * max(1, n))()
    mt = (abi.Meters * max(1, n))() if want_meters else None
    rc = load().icw_transcode_files_pool(C.byref(cfg), ptrs, cnt, byp, ins, outs, n, C.byref(o), C.byref(st), mt, status)
    meters = None
    if want_meters:
        meters = [{"clips": (m.clips[0], m.clips[1]), "peak_db": (m.peak_db[0], m.peak_db[1]), "desubnorm": m.desubnorm}
                  for m in list(mt)[:n]]
    return rc, st, [status[i] for i in range(n)], meters


def file_job(cfg, nodes):
    """icw_file_job_from_config: the job of a file that is to be transcoded as `cfg` (an abi.Config: its render,
    need24bits, Hilbert fields and bypass_list) with the list `nodes`; the FileJob keeps its node array alive"""
    arr = graph_nodes(nodes)
    job = abi.FileJob()
    load().icw_file_job_from_config(C.byref(cfg), arr, len(nodes), C.byref(job))
    job.keep_nodes = arr
    return job


def _job_array(jobs):
    arr = (abi.FileJob * max(1, len(jobs)))()
    for i, j in enumerate(jobs):
        arr[i] = j
    return arr


def file_job_classes(jobs, cwave=False):
    """icw_file_job_classes (host only): (number of classes, every job's class as its position in the layout of a
    pool context that holds these jobs; -1 for a job whose fields are out of range)"""
    n = len(jobs)
    cls = (C.c_int32 * max(1, n))()
    k = load().icw_file_job_classes(_job_array(jobs), n, int(bool(cwave)), cls)
    return k, [cls[i] for i in range(n)]


def pool_plan_classes(totals, classes, slots, block_frames=0, order=abi.POOL_AS_GIVEN):
    """icw_pool_plan_classes (host only): pool_plan with file i of class classes[i], every class in a contiguous
    range of slots of its own; returns (rc, per-file slots, per-file start blocks, JobsStats)"""
    n = len(totals)
    assert len(classes) == n
    tot = (C.c_int64 * max(1, n))(*[int(t) for t in totals])
    cls = (C.c_int32 * max(1, n))(*[int(c) for c in classes])
    slot = (C.c_int32 * max(1, n))()
    start = (C.c_int64 * max(1, n))()
    st = abi.JobsStats()
    rc = load().icw_pool_plan_classes(tot, cls, n, int(slots), int(block_frames), int(order), slot, start, C.byref(st))
    return rc, [slot[i] for i in range(n)], [start[i] for i in range(n)], st


def transcode_files_jobs(cfg, jobs, in_paths, out_paths, slots=0, order=abi.POOL_AS_GIVEN, fade_in_ms=0, fade_out_ms=0,
                         sec_align=0, block_frames=0, device=-1, timing=False, want_meters=True):
    """icw_transcode_files_jobs: transcode_files_pool with file i's own job (file_job: list, render and depth,
    Hilbert converter); cfg gives frmod_scaled and the seeds.  timing: ICW_BATCH_TIMING.  Returns (rc, JobsStats,
    per-file status, per-file meters as transcode_files_pool gives them)"""
    n = len(in_paths)
    assert len(jobs) == n and len(out_paths) == n
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    arr = _job_array(jobs)
    o = abi.PoolOpts(abi.BatchOpts(fade_in_ms, fade_out_ms, sec_align, block_frames, device,
                                   abi.BATCH_TIMING if timing else 0), int(slots), int(order))
    st = abi.JobsStats()
    status = (C.c_int * max(1, n))()
    mt = (abi.Meters * max(1, n))() if want_meters else None
    rc = load().icw_transcode_files_jobs(C.byref(cfg), arr, ins, outs, n, C.byref(o), C.byref(st), mt, status)
    meters = None
    if want_meters:
        meters = [{"clips": (m.clips[0], m.clips[1]), "peak_db": (m.peak_db[0], m.peak_db[1]), "desubnorm": m.desubnorm}
                  for m in list(mt)[:n]]
    return rc, st, [status[i] for i in range(n)], meters


def cwave_frame_bytes(cw_format, channels):
    """icw_cwave_frame_bytes: bytes of one CWAVE frame for an input of `channels` channels (0: invalid)"""
    return int(load().icw_cwave_frame_bytes(cw_format, channels))


def cwave_encode_files(in_paths, out_paths, k_M, k_beta=8.0, cw_format=abi.FMT_CW_F64, align=0, block_frames=0,
                       device=-1, merge_inputs=False):
    """icw_cwave_encode_files: WAV files to V2 CWAVE files through the FIR Hilbert converter; returns
    (rc, stats, per-file status, per-file clipped int16 samples).  merge_inputs: ICW_ENC_MERGE_INPUTS, every
    file in one context"""
    n = len(in_paths)
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    o = abi.CwaveEncOpts(k_M, align, k_beta, cw_format, block_frames, device, abi.ENC_MERGE_INPUTS if merge_inputs else 0)
    st = abi.BatchStats()
    status = (C.c_int * max(1, n))()
    clipped = (C.c_uint64 * max(1, n))()
    rc = load().icw_cwave_encode_files(ins, outs, n, C.byref(o), C.byref(st), clipped, status)
    return rc, st, [status[i] for i in range(n)], [int(clipped[i]) for i in range(n)]


def cwave_encode_files_iir(in_paths, out_paths, hilbert_type=1, iir_kahan=1, iir_subnorm_reject=1,
                           cw_format=abi.FMT_CW_F64, block_frames=0, device=-1, merge_inputs=False):
    """icw_cwave_encode_files_iir: WAV files to V2 CWAVE files (k_M 0) through the quadrature IIR converter;
    returns (rc, stats, per-file status, per-file clipped int16 samples).  merge_inputs: ICW_ENC_MERGE_INPUTS,
    every file in one context"""
    n = len(in_paths)
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    o = abi.CwaveEncIirOpts(hilbert_type, iir_kahan, iir_subnorm_reject, cw_format, block_frames, device,
                            abi.ENC_MERGE_INPUTS if merge_inputs else 0)
    st = abi.BatchStats()
    status = (C.c_int * max(1, n))()
    clipped = (C.c_uint64 * max(1, n))()
    rc = load().icw_cwave_encode_files_iir(ins, outs, n, C.byref(o), C.byref(st), clipped, status)
    return rc, st, [status[i] for i in range(n)], [int(clipped[i]) for i in range(n)]


def _u64(values):
    return (C.c_uint64 * max(1, len(values)))(*[int(v) for v in values])


def encode_cwave_fft_passes(n_frames, max_pass_log2=0):
    """icw_encode_cwave_fft_passes: passes per transform direction of a track of n_frames frames"""
    k = int(load().icw_encode_cwave_fft_passes(int(n_frames), int(max_pass_log2)))
    if k < 0:
        _check(k, "icw_encode_cwave_fft_passes")
    return k


def encode_cwave_fft_workspace(n_frames, channels=2):
    """icw_encode_cwave_fft_workspace: device working-set bytes of a call over tracks of n_frames[i] frames"""
    return int(load().icw_encode_cwave_fft_workspace(_u64(n_frames), len(n_frames), channels))


def encode_cwave_fft(tracks, fmt, channels, cw_format=abi.FMT_CW_F64, max_pass_log2=0, device=-1):
    """icw_encode_cwave_fft, host pointers: tracks is a list of uint8 arrays of whole PCM tracks (format fmt,
    `channels` interleaved channels) that go through the direct-FFT converter in ONE call.  Returns (list of
    uint8 arrays of packed CWAVE frames, list of clipped int16 samples)."""
    fsz = abi.FMT_BYTES[fmt] * channels
    fb = cwave_frame_bytes(cw_format, channels)
    tracks = [np.ascontiguousarray(t, dtype=np.uint8).reshape(-1) for t in tracks]
    nfr = [t.size // fsz for t in tracks]
    inp = np.concatenate(tracks) if tracks else np.zeros(1, np.uint8)
    ioff = np.concatenate([[0], np.cumsum([t.size for t in tracks])])[:-1] if tracks else []
    ooff = np.concatenate([[0], np.cumsum([n * fb for n in nfr])])[:-1] if tracks else []
    out = np.zeros(max(1, sum(nfr) * fb), dtype=np.uint8)
    clipped = _u64([0] * len(tracks))
    o = abi.FftEncOpts(device, max_pass_log2)
    _check(load().icw_encode_cwave_fft(_ptr(inp), _u64(ioff), _u64(nfr), len(tracks), fmt, channels, _ptr(out), _u64(ooff),
                                       cw_format, clipped, 0, C.byref(o), None), "icw_encode_cwave_fft")
    return ([out[int(b):int(b) + n * fb].copy() for b, n in zip(ooff, nfr)], [int(clipped[i]) for i in range(len(tracks))])


def encode_cwave_fft_device(d_in, in_offsets, n_frames, fmt, channels, d_out, out_offsets, cw_format=abi.FMT_CW_F64,
                            max_pass_log2=0, device=-1, hip_stream=None):
    """icw_encode_cwave_fft with ICW_F_DEVICE_PTRS (torch tensors / int pointers): track i's PCM at
    d_in + in_offsets[i], its frames to d_out + out_offsets[i].  Returns the clipped counts; the call has
    waited for hip_stream."""
    n = len(n_frames)
    clipped = _u64([0] * n)
    o = abi.FftEncOpts(device, max_pass_log2)
    _check(load().icw_encode_cwave_fft(_ptr(d_in), _u64(in_offsets), _u64(n_frames), n, fmt, channels, _ptr(d_out),
                                       _u64(out_offsets), cw_format, clipped, abi.F_DEVICE_PTRS, C.byref(o), hip_stream),
           "icw_encode_cwave_fft")
    return [int(clipped[i]) for i in range(n)]


def cwave_encode_files_fft(in_paths, out_paths, cw_format=abi.FMT_CW_F64, device=-1, max_bytes=0):
    """icw_cwave_encode_files_fft: WAV files to V2 CWAVE files (k_M -1) through the direct-FFT converter; returns
    (rc, stats, per-file status, per-file clipped int16 samples)"""
    n = len(in_paths)
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    o = abi.CwaveEncFftOpts(cw_format, device, max_bytes)
    st = abi.BatchStats()
    status = (C.c_int * max(1, n))()
    clipped = (C.c_uint64 * max(1, n))()
    rc = load().icw_cwave_encode_files_fft(ins, outs, n, C.byref(o), C.byref(st), clipped, status)
    return rc, st, [status[i] for i in range(n)], [int(clipped[i]) for i in range(n)]


def transcode_files_devices(cfg, nodes, in_paths, out_paths, devices, fade_in_ms=0, fade_out_ms=0, sec_align=0,
                            block_frames=0, merge_inputs=False, merge_cwave=False):
    """icw_transcode_files_devices: the files split over `devices` (one host thread each)"""
    n = len(in_paths)
    ins = (C.c_char_p * max(1, n))(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * max(1, n))(*[str(p).encode() for p in out_paths])
    arr = graph_nodes(nodes)
    o = abi.BatchOpts(fade_in_ms, fade_out_ms, sec_align, block_frames, -1,
                      _batch_flags(merge_inputs, merge_cwave))
    dv = (C.c_int * len(devices))(*devices)
    st = abi.BatchStats()
    status = (C.c_int * max(1, n))()
    rc = load().icw_transcode_files_devices(C.byref(cfg), arr, len(nodes), ins, outs, n, C.byref(o), dv,
                                            len(devices), C.byref(st), status)
    return rc, st, [status[i] for i in range(n)]


class Group:
    """icw_group: n_streams streams sharded over several devices, one context and one host
    thread per device (include/icw_group.h)"""

    def __init__(self, cfg, nodes, n_streams, devices):
        lib = load()
        self._lib = lib
        arr = graph_nodes(nodes)
        dv = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        acc = C.c_int()
        _check(lib.icw_group_create(C.byref(cfg), arr, len(nodes), n_streams, dv, len(devices), C.byref(h),
                                    C.byref(acc)), "icw_group_create")
        self.h, self.accepted, self.n_streams = h, bool(acc.value), n_streams
        self.fsz = abi.FMT_BYTES[cfg.in_format] * cfg.in_channels
        self.osz = 2 * (3 if cfg.need24bits else 2)

    def close(self):
        if self.h:
            self._lib.icw_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard(self, d):
        f, c, dev, ctx = C.c_int(), C.c_int(), C.c_int(), C.c_void_p()
        _check(self._lib.icw_group_shard(self.h, d, C.byref(f), C.byref(c), C.byref(dev), C.byref(ctx)),
               "icw_group_shard")
        return f.value, c.value, dev.value

    def process(self, inp, n_frames, want_pre=False, out=None):
        """out: an optional [n_streams, >= n_frames * osz] uint8 array (e.g. host_array: pinned, so every
        shard copies its slices block by block on its own device)"""
        inp = np.ascontiguousarray(inp)
        assert inp.dtype == np.uint8 and inp.shape[0] == self.n_streams and inp.shape[1] >= n_frames * self.fsz
        if out is None:
            out = np.zeros((self.n_streams, n_frames * self.osz), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.shape[0] == self.n_streams and out.shape[1] >= n_frames * self.osz
        pre = np.zeros((self.n_streams, n_frames, 2), dtype=np.float64) if want_pre else None
        _check(self._lib.icw_group_process(self.h, _ptr(inp), inp.strides[0], _ptr(out), out.strides[0], n_frames,
                                           abi.F_DEBUG_PRE if want_pre else 0, _ptr(pre)), "icw_group_process")
        return out, pre

    def meters(self, s, reset=False):
        m = abi.Meters()
        _check(self._lib.icw_group_get_meters(self.h, s, 1 if reset else 0, C.byref(m)), "icw_group_get_meters")
        return {"clips": (m.clips[0], m.clips[1]), "peak_db": (m.peak_db[0], m.peak_db[1]),
                "desubnorm": m.desubnorm}

    def n_frame(self, s):
        v = C.c_uint64()
        _check(self._lib.icw_group_n_frame(self.h, s, C.byref(v)), "icw_group_n_frame")
        return v.value


def graph_nodes(nodes):
    arr = (abi.Node * max(1, len(nodes)))()
    for i, nd in enumerate(nodes):
        arr[i] = nd
    return arr
