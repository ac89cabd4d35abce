"""ctypes binding to libhcodec.so (include/hcodec.h, include/hcodec_synth.h).

Host-side mirror of the reference's buffer-level interface (huffCompress / huffDecompress,
src/main.cpp:39-128) plus the batched device entry points. Torch is used only for device memory
and streams (tensors are passed by data_ptr()). There is deliberately no CPU fallback: if the
shared library is missing, every call raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
# HC_LIB_PATH: another build of the same library (A/B timing of kernel variants in one run)
LIB_PATH = os.environ.get("HC_LIB_PATH") or os.path.join(PKG, "lib", "libhcodec.so")
# the same sources built with the test / diagnostic hooks (-DHC_DEBUG_HOOKS): the hc_debug_*
# entry points exist only there, so the shipping library carries no mutable global state
DBG_LIB_PATH = os.environ.get("HC_DBG_LIB_PATH") or os.path.join(PKG, "lib", "libhcodec_dbg.so")
CLI_PATH = os.path.join(PKG, "bin", "huffman-codec")
BATCH_CLI_PATH = os.path.join(PKG, "bin", "huffman-codec-batch")
INCLUDE_DIR = os.path.join(os.path.dirname(PKG), "include")

HC_OK = 0
HC_ERR_WIDTH = 4
HC_ERR_MATRIX_SIZE = 6
HC_ERR_HEADER = 8
HC_ERR_HUFFMAN = 9
HC_ERR_ADAPT_HEADER = 10
HC_ERR_ADAPT_DIRS = 11
HC_ERR_DIMS = 12
HC_ERR_BLOCK_DATA = 13
HC_ERR_BLOCK_EOF = 14
HC_ERR_LEFTOVER = 15
HC_ERR_CAPACITY = 64
HC_ERR_UNSUPPORTED = 65
HC_ERR_BLOCK_SIZE = 66
HC_ERR_TOO_LARGE = 67
HC_ERR_SEG_HEADER = 68
HC_ERR_SEG_SIZE = 69
HC_ERR_DEVICE = 70
HC_ERR_ARG = 71
HC_ERR_SEG_CHECK = 72

HC_FLAG_DIFF = 0x80
HC_FLAG_ADAPT = 0x40
HC_SEG_CHECK_CRC32 = 0x100   # segmented encoders: a CRC-32 per segment; SegInfo.flags of a checked container
HC_SEG_DEFAULT_BYTES = 65536
NO_SEGMENT = 2**64 - 1   # bad_segment when no segment failed


class SegInfo(ctypes.Structure):
    """hc_seg_info_t: the header fields of a segmented container"""
    _fields_ = [("raw_len", ctypes.c_uint64), ("seg_bytes", ctypes.c_uint64), ("width", ctypes.c_uint64),
                ("n_segments", ctypes.c_uint64), ("flags", ctypes.c_uint32)]

HC_SEG_WHOLE = 2**64 - 1   # SegDecItem.length with offset 0: the whole container


class SegEncItem(ctypes.Structure):
    """hc_seg_enc_item_t: one input of a batched segmented encode"""
    _fields_ = [("in_off", ctypes.c_uint64), ("in_len", ctypes.c_uint64), ("width", ctypes.c_uint64),
                ("out_off", ctypes.c_uint64), ("out_cap", ctypes.c_uint64)]


class SegDecItem(ctypes.Structure):
    """hc_seg_dec_item_t: one container and one range of it (0, HC_SEG_WHOLE: the whole)"""
    _fields_ = [("in_off", ctypes.c_uint64), ("in_len", ctypes.c_uint64), ("info", SegInfo),
                ("offset", ctypes.c_uint64), ("length", ctypes.c_uint64),
                ("out_off", ctypes.c_uint64), ("out_cap", ctypes.c_uint64)]


class SegPatch(ctypes.Structure):
    """hc_seg_patch_t: raw bytes [offset, offset + length) become patch_data[src_off .. src_off + length)"""
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint64), ("src_off", ctypes.c_uint64)]


class SegRead(ctypes.Structure):
    """hc_seg_read_t: raw bytes [offset, offset + length) go to out[dst_off .. dst_off + length)"""
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint64), ("dst_off", ctypes.c_uint64)]


SYNTH = {"noise": 0, "grad": 1, "photo": 2}

_libs = {}           # path -> loaded library
_active = LIB_PATH   # the library every call below goes to (use_debug_build switches it)


class HCodecError(RuntimeError):
    pass


def build():
    import subprocess
    subprocess.run(["make", "-s", "-C", PKG], check=True)


def use_debug_build(on=True):
    """Route every later call of this module to libhcodec_dbg.so (on) or back to the shipping
    libhcodec.so (off). Tests that set a debug hook run their calls on the debug build; the two
    libraries are separate code objects, each with its own device state."""
    global _active
    _active = DBG_LIB_PATH if on else LIB_PATH
    return lib()


def lib():
    """The active library (libhcodec.so unless use_debug_build); raise if it has not been built
    (no fallback path exists)."""
    return _load(_active)


def _load(path):
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise HCodecError(f"{path} missing: build it with `make -C {PKG}`")
    # torch ships its own libamdhip64.so.7 (same soname as /opt/rocm's). Whichever loads first
    # serves the whole process; loading ours first leaves torch without a GPU. So let torch's
    # runtime load first and libhcodec.so binds to it: one HIP runtime, shared device pointers.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    u8p = ctypes.c_void_p
    u64 = ctypes.c_uint64
    vp = ctypes.c_void_p
    L.hc_compress_bound.argtypes = [u64, ctypes.c_int]
    L.hc_compress_bound.restype = u64
    L.hc_compress.argtypes = [u8p, u64, ctypes.c_int, ctypes.c_int, u64, u8p, u64,
                              ctypes.POINTER(u64)]
    L.hc_decompress.argtypes = [u8p, u64, u8p, u64, ctypes.POINTER(u64)]
    L.hc_decompress_alloc.argtypes = [u8p, u64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u64)]
    L.hc_free.argtypes = [vp]
    L.hc_compress_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp,
                                    vp, vp]
    L.hc_compress_batch_aux.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp,
                                        vp, vp, vp]
    L.hc_decompress_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    L.hc_compress_host_batch.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp]
    L.hc_decompress_host_batch.argtypes = [vp, vp, ctypes.c_uint32, vp, vp, vp, vp]
    L.hc_compress_adapt_host_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp]
    L.hc_adapt_compress_work_bound.argtypes = [u64, ctypes.c_uint32]
    L.hc_adapt_compress_work_bound.restype = u64
    L.hc_adapt_decompress_work_bound.argtypes = [u64, u64, ctypes.c_uint32]
    L.hc_adapt_decompress_work_bound.restype = u64
    L.hc_compress_adapt_batch.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, vp,
                                          vp, u64, vp]
    L.hc_decompress_adapt_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, u64, vp]
    L.hc_pack_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp]
    L.hc_version.restype = ctypes.c_char_p
    L.hc_device_ok.restype = ctypes.c_int
    L.hc_device_info.argtypes = [ctypes.c_char_p, u64]
    L.hc_device_info.restype = ctypes.c_int
    L.hc_synth_batch.argtypes = [ctypes.c_int, u64, ctypes.c_uint32, u64, u64, vp, u64, vp]
    for f in (L.hc_seg_count, L.hc_seg_compress_bound, L.hc_seg_compress_work_bound):
        f.argtypes = [u64, u64, ctypes.c_int, u64]
        f.restype = u64
    for f in (L.hc_seg_compress_bound2, L.hc_seg_compress_work_bound2):
        f.argtypes = [u64, u64, ctypes.c_uint32, u64]
        f.restype = u64
    L.hc_seg_compress2.argtypes = [u8p, u64, ctypes.c_uint32, u64, u64, u8p, u64, ctypes.POINTER(u64)]
    L.hc_crc32_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp]
    L.hc_seg_info.argtypes = [u8p, u64, ctypes.POINTER(SegInfo)]
    L.hc_seg_compress.argtypes = [u8p, u64, ctypes.c_int, ctypes.c_int, u64, u64, u8p, u64, ctypes.POINTER(u64)]
    L.hc_seg_decompress.argtypes = [u8p, u64, u8p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.hc_seg_decompress_alloc.argtypes = [u8p, u64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u64),
                                          ctypes.POINTER(u64)]
    L.hc_seg_compress_dev.argtypes = [vp, u64, ctypes.c_uint32, u64, u64, vp, u64, vp, vp, vp, u64, vp]
    L.hc_seg_decompress_work_bound.argtypes = [ctypes.POINTER(SegInfo), u64]
    L.hc_seg_decompress_work_bound.restype = u64
    L.hc_seg_decompress_dev.argtypes = [vp, u64, ctypes.POINTER(SegInfo), vp, u64, vp, vp, vp, vp, u64, vp]
    L.hc_seg_range_segments.argtypes = [ctypes.POINTER(SegInfo), u64, u64, u64, ctypes.POINTER(u64),
                                        ctypes.POINTER(u64)]
    L.hc_seg_decompress_range.argtypes = [u8p, u64, u64, u64, u8p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.hc_seg_decompress_range_work_bound.argtypes = [ctypes.POINTER(SegInfo), u64, u64, u64]
    L.hc_seg_decompress_range_work_bound.restype = u64
    L.hc_seg_decompress_range_dev.argtypes = [vp, u64, ctypes.POINTER(SegInfo), u64, u64, vp, u64, vp, vp, vp, vp, u64,
                                              vp]
    pp = ctypes.POINTER(SegPatch)
    L.hc_seg_update_segments.argtypes = [ctypes.POINTER(SegInfo), u64, pp, ctypes.c_uint32, ctypes.POINTER(u64),
                                         ctypes.POINTER(u64)]
    for f in (L.hc_seg_update_bound, L.hc_seg_update_work_bound):
        f.argtypes = [ctypes.POINTER(SegInfo), u64, pp, ctypes.c_uint32]
        f.restype = u64
    L.hc_seg_update_dev.argtypes = [vp, u64, ctypes.POINTER(SegInfo), pp, ctypes.c_uint32, vp, u64, vp, u64, vp, vp, vp,
                                    vp, u64, vp]
    L.hc_seg_update.argtypes = [u8p, u64, pp, ctypes.c_uint32, u8p, u64, u8p, u64, ctypes.POINTER(u64),
                                ctypes.POINTER(u64)]
    rp = ctypes.POINTER(SegRead)
    L.hc_seg_reads_segments.argtypes = [ctypes.POINTER(SegInfo), u64, rp, ctypes.c_uint32, ctypes.POINTER(u64),
                                        ctypes.POINTER(u64)]
    L.hc_seg_decompress_ranges_work_bound.argtypes = [ctypes.POINTER(SegInfo), u64, rp, ctypes.c_uint32]
    L.hc_seg_decompress_ranges_work_bound.restype = u64
    L.hc_seg_decompress_ranges_dev.argtypes = [vp, u64, ctypes.POINTER(SegInfo), rp, ctypes.c_uint32, vp, u64, vp, vp, vp,
                                               vp, u64, vp]
    L.hc_seg_decompress_ranges.argtypes = [u8p, u64, rp, ctypes.c_uint32, u8p, u64, ctypes.POINTER(u64),
                                           ctypes.POINTER(u64)]
    L.hc_seg_rect_reads.argtypes = [u64, u64, u64, u64, u64, u64, rp]
    L.hc_seg_append_plan.argtypes = [ctypes.POINTER(SegInfo), u64, u64, ctypes.POINTER(SegInfo), ctypes.POINTER(u64),
                                     ctypes.POINTER(u64)]
    for f in (L.hc_seg_append_bound, L.hc_seg_append_work_bound):
        f.argtypes = [ctypes.POINTER(SegInfo), u64, u64]
        f.restype = u64
    L.hc_seg_append_dev.argtypes = [vp, u64, ctypes.POINTER(SegInfo), vp, u64, vp, u64, vp, vp, vp, vp, u64, vp]
    L.hc_seg_append.argtypes = [u8p, u64, u8p, u64, u8p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.hc_seg_compress_batch_work_bound.argtypes = [ctypes.POINTER(SegEncItem), ctypes.c_uint32, ctypes.c_uint32, u64]
    L.hc_seg_compress_batch_work_bound.restype = u64
    L.hc_seg_compress_batch_dev.argtypes = [vp, vp, ctypes.POINTER(SegEncItem), ctypes.c_uint32, ctypes.c_uint32, u64,
                                            vp, vp, vp, u64, vp]
    L.hc_seg_decompress_batch_work_bound.argtypes = [ctypes.POINTER(SegDecItem), ctypes.c_uint32]
    L.hc_seg_decompress_batch_work_bound.restype = u64
    L.hc_seg_decompress_batch_dev.argtypes = [vp, vp, ctypes.POINTER(SegDecItem), ctypes.c_uint32, vp, vp, vp, vp, u64,
                                              vp]
    L.hc_seg_compress_host_batch.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, u64, vp, vp, vp, vp]
    L.hc_seg_decompress_host_batch.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
    _libs[path] = L
    return L


def _dbg():
    """the debug build, which must be the active one (a hook set there would otherwise not
    affect the calls that follow)"""
    if _active != DBG_LIB_PATH:
        raise HCodecError("debug hooks need use_debug_build(True) first")
    return lib()


def release_cached():
    """hc_release_cached: free the library's cached device / pinned buffers"""
    lib().hc_release_cached()


def _buf(data):
    b = bytes(data)
    return b, ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) if b else None


def compress(data, use_diff=False, use_adapt=False, width=512):
    """hc_compress: (status, encoded bytes). Mirrors huffCompress (main.cpp:39-87)."""
    b, p = _buf(data)
    cap = lib().hc_compress_bound(len(b), int(bool(use_adapt)))
    out = ctypes.create_string_buffer(max(int(cap), 1))
    n = ctypes.c_uint64(0)
    st = lib().hc_compress(p, len(b), int(bool(use_diff)), int(bool(use_adapt)), width,
                           ctypes.cast(out, ctypes.c_void_p), cap, ctypes.byref(n))
    return st, (out.raw[:n.value] if st == 0 else b"")


def decompress(data):
    """hc_decompress_alloc: (status, decoded bytes). Mirrors huffDecompress (main.cpp:90-128)."""
    b, p = _buf(data)
    q = ctypes.c_void_p()
    n = ctypes.c_uint64(0)
    st = lib().hc_decompress_alloc(p, len(b), ctypes.byref(q), ctypes.byref(n))
    out = b""
    if st == 0:
        out = ctypes.string_at(q, n.value) if n.value else b""
    if q:
        lib().hc_free(q)
    return st, out


def _stream_handle(stream):
    if stream is None:
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


def _dp(t):
    return ctypes.c_void_p(t.data_ptr())


def _check_batch(inp, in_offs, in_lens, out, out_offs, out_caps, out_lens, status):
    """The batch entry points take raw device pointers: a CPU, non-contiguous or wrongly typed
    tensor would become an out-of-bounds device access, so reject it here instead."""
    import torch
    n = in_offs.numel()
    spec = (("in", inp, torch.uint8, None), ("in_offs", in_offs, torch.int64, n),
            ("in_lens", in_lens, torch.int64, n), ("out", out, torch.uint8, None),
            ("out_offs", out_offs, torch.int64, n), ("out_caps", out_caps, torch.int64, n),
            ("out_lens", out_lens, torch.int64, n), ("status", status, torch.int32, n))
    dev = inp.device
    for name, t, dt, numel in spec:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch tensor")
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{name}: expected a CUDA tensor on {dev}, got {t.device}")
        if t.dtype != dt:
            raise TypeError(f"{name}: expected {dt}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
        if numel is not None and t.numel() != numel:
            raise ValueError(f"{name}: {t.numel()} entries for {n} streams")
    return n


_AUX = {}  # device index -> a side stream for the encoder's table-mode launches (Python-side)


def _aux_stream(inp):
    import torch
    d = inp.device.index if inp.device.index is not None else torch.cuda.current_device()
    if d not in _AUX:
        _AUX[d] = torch.cuda.Stream(device=d)
    return _AUX[d]


def compress_batch(inp, in_offs, in_lens, out, out_offs, out_caps, out_lens, status,
                   use_diff=False, stream=None, aux_stream="auto"):
    """hc_compress_batch_aux on torch CUDA tensors (uint8 data, int64 offsets/lengths, int32
    status). aux_stream: a second stream for the table-mode launches ("auto": one side stream
    per device kept by this module; None: both modes one after the other on `stream`)."""
    n = _check_batch(inp, in_offs, in_lens, out, out_offs, out_caps, out_lens, status)
    aux = _aux_stream(inp) if aux_stream == "auto" else aux_stream
    rc = lib().hc_compress_batch_aux(_dp(inp), _dp(in_offs), _dp(in_lens), n,
                                     HC_FLAG_DIFF if use_diff else 0, _dp(out), _dp(out_offs),
                                     _dp(out_caps), _dp(out_lens), _dp(status), _stream_handle(stream),
                                     ctypes.c_void_p(None) if aux is None else _stream_handle(aux))
    if rc:
        raise HCodecError(f"hc_compress_batch failed: {rc}")


def decompress_batch(inp, in_offs, in_lens, out, out_offs, out_caps, out_lens, status, stream=None):
    """hc_decompress_batch on torch CUDA tensors (same layout as compress_batch)."""
    n = _check_batch(inp, in_offs, in_lens, out, out_offs, out_caps, out_lens, status)
    rc = lib().hc_decompress_batch(_dp(inp), _dp(in_offs), _dp(in_lens), n, _dp(out),
                                   _dp(out_offs), _dp(out_caps), _dp(out_lens), _dp(status),
                                   _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_decompress_batch failed: {rc}")


def _work(nbytes, device):
    import torch
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _check_work(work, device, need):
    import torch
    if not (isinstance(work, torch.Tensor) and work.is_cuda and work.device == device
            and work.dtype == torch.uint8 and work.is_contiguous()):
        raise ValueError(f"work: expected a contiguous uint8 CUDA tensor on {device}")
    if work.data_ptr() % 16:
        raise ValueError("work: must be 16-byte aligned")
    if work.numel() < need:
        raise ValueError(f"work: {work.numel()} bytes, the call needs {need}")


def compress_adapt_batch(inp, in_offs, in_lens, widths, out, out_offs, out_caps, out_lens, status,
                         use_diff=False, stream=None, work=None):
    """hc_compress_adapt_batch (-a, optionally -m) on CUDA tensors; widths: int64 per matrix.
    The workspace is allocated here unless given (uint8 CUDA tensor)."""
    n = _check_batch(inp, in_offs, in_lens, out, out_offs, out_caps, out_lens, status)
    _check_batch(inp, in_offs, widths, out, out_offs, out_caps, out_lens, status)
    need = int(lib().hc_adapt_compress_work_bound(int(in_lens.sum()), n))
    if work is None:
        work = _work(need, inp.device)
    _check_work(work, inp.device, need)
    rc = lib().hc_compress_adapt_batch(_dp(inp), _dp(in_offs), _dp(in_lens), _dp(widths), n,
                                       HC_FLAG_DIFF if use_diff else 0, _dp(out), _dp(out_offs), _dp(out_caps),
                                       _dp(out_lens), _dp(status), _dp(work), work.numel(),
                                       _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_compress_adapt_batch failed: {rc}")
    return work


def decompress_adapt_batch(inp, in_offs, in_lens, out, out_offs, out_caps, out_lens, status, stream=None,
                           work=None):
    """hc_decompress_adapt_batch on CUDA tensors (adaptive streams -> matrices)."""
    n = _check_batch(inp, in_offs, in_lens, out, out_offs, out_caps, out_lens, status)
    need = int(lib().hc_adapt_decompress_work_bound(int(in_lens.sum()), int(out_caps.sum()), n))
    if work is None:
        work = _work(need, inp.device)
    _check_work(work, inp.device, need)
    rc = lib().hc_decompress_adapt_batch(_dp(inp), _dp(in_offs), _dp(in_lens), n, _dp(out), _dp(out_offs),
                                         _dp(out_caps), _dp(out_lens), _dp(status), _dp(work), work.numel(),
                                         _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_decompress_adapt_batch failed: {rc}")
    return work


def seg_count(n, seg_bytes=0, use_adapt=False, width=512):
    """hc_seg_count: segments of an n-byte input (0: invalid arguments)"""
    return int(lib().hc_seg_count(n, seg_bytes, int(bool(use_adapt)), width))


def _seg_flags(use_diff, use_adapt, check):
    return (HC_FLAG_DIFF if use_diff else 0) | (HC_FLAG_ADAPT if use_adapt else 0) | (HC_SEG_CHECK_CRC32 if check else 0)


def seg_compress_bound(n, seg_bytes=0, use_adapt=False, width=512, check=False):
    """hc_seg_compress_bound2: the worst-case container size (check: with a CRC-32 per segment)"""
    return int(lib().hc_seg_compress_bound2(n, seg_bytes, _seg_flags(False, use_adapt, check), width))


def seg_info(data):
    """hc_seg_info (host only, no device): (status, SegInfo or None) of a container's header"""
    b, p = _buf(data)
    info = SegInfo()
    st = lib().hc_seg_info(p, len(b), ctypes.byref(info))
    return st, (info if st == 0 else None)


def seg_compress(data, use_diff=False, use_adapt=False, width=512, seg_bytes=0, cap=None, check=False):
    """hc_seg_compress2: (status, HCSEG1 container) of one input coded as parallel segments.
    cap: the output capacity (default: hc_seg_compress_bound2). check: store a CRC-32 of every
    segment's raw bytes in the index; the decoders verify it."""
    b, p = _buf(data)
    flags = _seg_flags(use_diff, use_adapt, check)
    if cap is None:
        cap = lib().hc_seg_compress_bound2(len(b), seg_bytes if seg_bytes % 16 == 0 else 0, flags, width)
    out = ctypes.create_string_buffer(max(int(cap), 1))
    n = ctypes.c_uint64(0)
    st = lib().hc_seg_compress2(p, len(b), flags, width, seg_bytes, ctypes.cast(out, ctypes.c_void_p), cap,
                                ctypes.byref(n))
    return st, (out.raw[:n.value] if st == 0 else b"")


def seg_decompress(data, full=False):
    """hc_seg_decompress_alloc: (status, decoded bytes); full: (status, bytes, out_len, bad_segment)"""
    b, p = _buf(data)
    q = ctypes.c_void_p()
    n = ctypes.c_uint64(0)
    bad = ctypes.c_uint64(0)
    st = lib().hc_seg_decompress_alloc(p, len(b), ctypes.byref(q), ctypes.byref(n), ctypes.byref(bad))
    out = b""
    if st == 0:
        out = ctypes.string_at(q, n.value) if n.value else b""
    if q:
        lib().hc_free(q)
    return (st, out, n.value, bad.value) if full else (st, out)


def _check_seg(inp, out, out_len, status, bad_segment):
    """the tensor checks of _check_batch for the segmented device calls (one result each)"""
    import torch
    spec = [("in", inp, torch.uint8, None), ("out", out, torch.uint8, None), ("out_len", out_len, torch.int64, 1),
            ("status", status, torch.int32, 1)]
    if bad_segment is not None:
        spec.append(("bad_segment", bad_segment, torch.int64, 1))
    dev = inp.device if isinstance(inp, torch.Tensor) else None
    for name, t, dt, numel in spec:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch tensor")
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{name}: expected a CUDA tensor on {dev}, got {t.device}")
        if t.dtype != dt:
            raise TypeError(f"{name}: expected {dt}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
        if numel is not None and t.numel() != numel:
            raise ValueError(f"{name}: {t.numel()} entries, expected {numel}")
    for name, t in (("in", inp), ("out", out)):
        if t.data_ptr() % 16:
            raise ValueError(f"{name}: must be 16-byte aligned")


def seg_compress_dev(inp, out, out_len, status, use_diff=False, use_adapt=False, width=512, seg_bytes=0,
                     stream=None, work=None, out_cap=None, check=False):
    """hc_seg_compress_dev on CUDA tensors: the whole of `inp` (uint8) into one container in `out`
    (capacity out_cap, default all of it); out_len (int64[1]) and status (int32[1]) are device
    results, asynchronous on `stream`. check: a checked container (a CRC-32 per segment). The
    workspace is allocated here unless given. Returns it."""
    _check_seg(inp, out, out_len, status, None)
    cap = out.numel() if out_cap is None else int(out_cap)
    if cap > out.numel():
        raise ValueError(f"out_cap {cap} exceeds the {out.numel()}-byte output tensor")
    flags = _seg_flags(use_diff, use_adapt, check)
    need = int(lib().hc_seg_compress_work_bound2(inp.numel(), seg_bytes, flags, width))
    if work is None:
        work = _work(need, inp.device)
    _check_work(work, inp.device, need)
    rc = lib().hc_seg_compress_dev(_dp(inp), inp.numel(), flags, width, seg_bytes, _dp(out), cap, _dp(out_len),
                                   _dp(status), _dp(work), work.numel(), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_seg_compress_dev failed: {rc}")
    return work


def seg_decompress_dev(inp, out, out_len, status, bad_segment=None, info=None, stream=None, work=None,
                       in_len=None, out_cap=None):
    """hc_seg_decompress_dev on CUDA tensors: the container in inp[:in_len] into `out` (capacity
    out_cap, default all of it). info: the container's SegInfo; when not given, the 48 header
    bytes are copied down (a synchronising copy) and parsed here; a header that does not parse
    is passed on as it is and the device status reports HC_ERR_SEG_HEADER. Returns the workspace."""
    _check_seg(inp, out, out_len, status, bad_segment)
    n = inp.numel() if in_len is None else int(in_len)
    if n > inp.numel():
        raise ValueError(f"in_len {n} exceeds the {inp.numel()}-byte input tensor")
    cap = out.numel() if out_cap is None else int(out_cap)
    if cap > out.numel():
        raise ValueError(f"out_cap {cap} exceeds the {out.numel()}-byte output tensor")
    if info is None:
        head, p = _buf(inp[:min(n, 48)].cpu().numpy().tobytes())
        info = SegInfo()  # stays all zero when the header does not parse: the call rejects it
        lib().hc_seg_info(p, n, ctypes.byref(info))
    need = int(lib().hc_seg_decompress_work_bound(ctypes.byref(info), n))
    if work is None:
        work = _work(need, inp.device)
    _check_work(work, inp.device, need)
    rc = lib().hc_seg_decompress_dev(_dp(inp), n, ctypes.byref(info), _dp(out), cap, _dp(out_len), _dp(status),
                                     ctypes.c_void_p(None) if bad_segment is None else _dp(bad_segment),
                                     _dp(work), work.numel(), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_seg_decompress_dev failed: {rc}")
    return work


def seg_range_segments(info, in_len, offset, length):
    """hc_seg_range_segments (host only, no device): (status, first, count) of the segments that
    hold raw bytes [offset, offset + length) of a container with this SegInfo"""
    first = ctypes.c_uint64(0)
    count = ctypes.c_uint64(0)
    st = lib().hc_seg_range_segments(ctypes.byref(info) if info is not None else None, in_len, offset, length,
                                     ctypes.byref(first), ctypes.byref(count))
    return st, first.value, count.value


def seg_decompress_range(data, offset, length, full=False, cap=None):
    """hc_seg_decompress_range: (status, raw bytes [offset, offset + length) of the container);
    full: (status, bytes, out_len, bad_segment). cap: the output capacity (default: length). Only
    the header, the index and the covered segments are uploaded."""
    b, p = _buf(data)
    if cap is None:
        cap = length
    out = ctypes.create_string_buffer(max(int(cap), 1))
    n = ctypes.c_uint64(0)
    bad = ctypes.c_uint64(NO_SEGMENT)
    st = lib().hc_seg_decompress_range(p, len(b), offset, length, ctypes.cast(out, ctypes.c_void_p), cap,
                                       ctypes.byref(n), ctypes.byref(bad))
    got = out.raw[:n.value] if st == 0 else b""
    return (st, got, n.value, bad.value) if full else (st, got)


def seg_decompress_range_dev(inp, out, out_len, status, offset, length, bad_segment=None, info=None, stream=None,
                             work=None, in_len=None, out_cap=None):
    """hc_seg_decompress_range_dev on CUDA tensors: raw bytes [offset, offset + length) of the
    container in inp[:in_len] into out[:length] (capacity out_cap, default all of `out`). info as
    for seg_decompress_dev. A range outside the container's raw_len raises. Returns the workspace."""
    _check_seg(inp, out, out_len, status, bad_segment)
    n = inp.numel() if in_len is None else int(in_len)
    if n > inp.numel():
        raise ValueError(f"in_len {n} exceeds the {inp.numel()}-byte input tensor")
    cap = out.numel() if out_cap is None else int(out_cap)
    if cap > out.numel():
        raise ValueError(f"out_cap {cap} exceeds the {out.numel()}-byte output tensor")
    if info is None:
        head, p = _buf(inp[:min(n, 48)].cpu().numpy().tobytes())
        info = SegInfo()  # stays all zero when the header does not parse: the call rejects it
        lib().hc_seg_info(p, n, ctypes.byref(info))
    need = int(lib().hc_seg_decompress_range_work_bound(ctypes.byref(info), n, offset, length))
    if work is None:
        work = _work(need, inp.device)
    _check_work(work, inp.device, need)
    rc = lib().hc_seg_decompress_range_dev(_dp(inp), n, ctypes.byref(info), offset, length, _dp(out), cap,
                                           _dp(out_len), _dp(status),
                                           ctypes.c_void_p(None) if bad_segment is None else _dp(bad_segment),
                                           _dp(work), work.numel(), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_seg_decompress_range_dev failed: {rc}")
    return work


def seg_patches(patches):
    """a ctypes array of SegPatch from (offset, length, src_off) triples (None when there are none)"""
    patches = list(patches)
    if not patches:
        return None
    return (SegPatch * len(patches))(*[SegPatch(o, m, s) for o, m, s in patches])


def seg_update_segments(info, in_len, patches):
    """hc_seg_update_segments (host only, no device): (status, covered, decoded) segment counts of
    a list of (offset, length, src_off) patches"""
    cov = ctypes.c_uint64(0)
    dec = ctypes.c_uint64(0)
    st = lib().hc_seg_update_segments(ctypes.byref(info) if info is not None else None, in_len, seg_patches(patches),
                                      len(patches), ctypes.byref(cov), ctypes.byref(dec))
    return st, cov.value, dec.value


def seg_update_bound(info, in_len, patches):
    """hc_seg_update_bound: an output capacity that always suffices (0: the call refuses the arguments)"""
    return int(lib().hc_seg_update_bound(ctypes.byref(info) if info is not None else None, in_len,
                                         seg_patches(patches), len(patches)))


def seg_update_work_bound(info, in_len, patches):
    """hc_seg_update_work_bound: the device call's workspace (0: refused; 16: an info that fails)"""
    return int(lib().hc_seg_update_work_bound(ctypes.byref(info) if info is not None else None, in_len,
                                              seg_patches(patches), len(patches)))


def seg_update(data, patches, full=False, cap=None):
    """hc_seg_update: (status, the container `data` with the (offset, bytes) patches written into
    its raw bytes); full: (status, bytes, out_len, bad_segment). cap: the output capacity (default:
    hc_seg_update_bound). The patches must be sorted by offset and must not overlap."""
    b, p = _buf(data)
    tri, blob, at = [], bytearray(), 0
    for o, pb in patches:
        tri.append((o, len(pb), at))
        blob += bytes(pb)
        at += len(pb)
    pd, pp = _buf(blob)
    arr = seg_patches(tri)
    if cap is None:
        st, info = seg_info(b)
        cap = seg_update_bound(info, len(b), tri) if st == 0 else 0
    out = ctypes.create_string_buffer(max(int(cap), 1))
    n = ctypes.c_uint64(0)
    bad = ctypes.c_uint64(NO_SEGMENT)
    st = lib().hc_seg_update(p, len(b), arr, len(tri), pp, len(pd), ctypes.cast(out, ctypes.c_void_p), cap,
                             ctypes.byref(n), ctypes.byref(bad))
    got = out.raw[:n.value] if st == 0 else b""
    return (st, got, n.value, bad.value) if full else (st, got)


def seg_update_dev(inp, patches, patch_data, out, out_len, status, bad_segment=None, info=None, stream=None,
                   work=None, in_len=None, out_cap=None, patch_data_len=None):
    """hc_seg_update_dev on CUDA tensors: the container in inp[:in_len] with the (offset, length,
    src_off) patches, whose bytes lie in the uint8 tensor patch_data (any alignment), into `out`
    (capacity out_cap, default all of it). info as for seg_decompress_dev. A patch list that fails
    its rules raises. Returns the workspace."""
    _check_seg(inp, out, out_len, status, bad_segment)
    import torch
    if not isinstance(patch_data, torch.Tensor) or patch_data.dtype != torch.uint8 or not patch_data.is_contiguous() \
            or patch_data.device != inp.device:
        raise TypeError("patch_data: expected a contiguous uint8 tensor on the input's device")
    n = inp.numel() if in_len is None else int(in_len)
    if n > inp.numel():
        raise ValueError(f"in_len {n} exceeds the {inp.numel()}-byte input tensor")
    cap = out.numel() if out_cap is None else int(out_cap)
    if cap > out.numel():
        raise ValueError(f"out_cap {cap} exceeds the {out.numel()}-byte output tensor")
    pdl = patch_data.numel() if patch_data_len is None else int(patch_data_len)
    if pdl > patch_data.numel():
        raise ValueError(f"patch_data_len {pdl} exceeds the {patch_data.numel()}-byte tensor")
    if info is None:
        head, p = _buf(inp[:min(n, 48)].cpu().numpy().tobytes())
        info = SegInfo()  # stays all zero when the header does not parse: the call rejects it
        lib().hc_seg_info(p, n, ctypes.byref(info))
    patches = list(patches)
    arr = seg_patches(patches)
    need = int(lib().hc_seg_update_work_bound(ctypes.byref(info), n, arr, len(patches)))
    if work is None:
        work = _work(need, inp.device)
    _check_work(work, inp.device, need)
    rc = lib().hc_seg_update_dev(_dp(inp), n, ctypes.byref(info), arr, len(patches),
                                 _dp(patch_data) if pdl else ctypes.c_void_p(None), pdl, _dp(out), cap, _dp(out_len),
                                 _dp(status), ctypes.c_void_p(None) if bad_segment is None else _dp(bad_segment),
                                 _dp(work), work.numel(), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_seg_update_dev failed: {rc}")
    return work


def seg_reads(reads):
    """a ctypes array of SegRead from (offset, length, dst_off) triples (None when there are none)"""
    reads = list(reads)
    if not reads:
        return None
    return (SegRead * len(reads))(*[SegRead(o, m, d) for o, m, d in reads])


def seg_reads_segments(info, in_len, reads):
    """hc_seg_reads_segments (host only, no device): (status, covered segments, need) of a list of
    (offset, length, dst_off) reads; need is the output bytes the list reaches"""
    cov = ctypes.c_uint64(0)
    need = ctypes.c_uint64(0)
    st = lib().hc_seg_reads_segments(ctypes.byref(info) if info is not None else None, in_len, seg_reads(reads),
                                     len(reads), ctypes.byref(cov), ctypes.byref(need))
    return st, cov.value, need.value


def seg_decompress_ranges_work_bound(info, in_len, reads):
    """hc_seg_decompress_ranges_work_bound: the device call's workspace (0: refused; 16: an info that fails)"""
    return int(lib().hc_seg_decompress_ranges_work_bound(ctypes.byref(info) if info is not None else None, in_len,
                                                         seg_reads(reads), len(reads)))


def seg_rect_reads(raw_len, pitch, x, y, w, h):
    """hc_seg_rect_reads (host only): (status, the (offset, length, dst_off) reads of the rows of the
    w x h rectangle at column x, row y of raw bytes read as rows of `pitch` bytes)"""
    arr = (SegRead * max(int(h), 1))() if h < 2**32 else None
    st = lib().hc_seg_rect_reads(raw_len, pitch, x, y, w, h, arr)
    return st, ([(r.offset, r.length, r.dst_off) for r in arr[:h]] if st == 0 else [])


def seg_decompress_ranges(data, reads, full=False, cap=None, fill=0):
    """hc_seg_decompress_ranges: (status, out[:need]) with the (offset, length, dst_off) reads of the
    container's raw bytes at their destinations and every other byte `fill`; full: (status, bytes,
    out_len, bad_segment). cap: the output capacity (default: need). The reads must be sorted by
    offset; each covered segment is uploaded and decoded once."""
    b, p = _buf(data)
    reads = list(reads)
    arr = seg_reads(reads)
    if cap is None:
        st, info = seg_info(b)
        cap = seg_reads_segments(info, len(b), reads)[2] if st == 0 else 0
    out = ctypes.create_string_buffer(bytes([fill]) * max(int(cap), 1), max(int(cap), 1))
    n = ctypes.c_uint64(0)
    bad = ctypes.c_uint64(NO_SEGMENT)
    st = lib().hc_seg_decompress_ranges(p, len(b), arr, len(reads), ctypes.cast(out, ctypes.c_void_p), cap,
                                        ctypes.byref(n), ctypes.byref(bad))
    got = out.raw[:n.value] if st == 0 else b""
    return (st, got, n.value, bad.value) if full else (st, got)


def seg_decompress_ranges_dev(inp, reads, out, out_len, status, bad_segment=None, info=None, stream=None, work=None,
                              in_len=None, out_cap=None):
    """hc_seg_decompress_ranges_dev on CUDA tensors: the (offset, length, dst_off) reads of the
    container in inp[:in_len] into `out` (capacity out_cap, default all of it). info as for
    seg_decompress_dev. A read list that fails its rules raises. Returns the workspace."""
    _check_seg(inp, out, out_len, status, bad_segment)
    n = inp.numel() if in_len is None else int(in_len)
    if n > inp.numel():
        raise ValueError(f"in_len {n} exceeds the {inp.numel()}-byte input tensor")
    cap = out.numel() if out_cap is None else int(out_cap)
    if cap > out.numel():
        raise ValueError(f"out_cap {cap} exceeds the {out.numel()}-byte output tensor")
    if info is None:
        head, p = _buf(inp[:min(n, 48)].cpu().numpy().tobytes())
        info = SegInfo()  # stays all zero when the header does not parse: the call rejects it
        lib().hc_seg_info(p, n, ctypes.byref(info))
    reads = list(reads)
    arr = seg_reads(reads)
    need = int(lib().hc_seg_decompress_ranges_work_bound(ctypes.byref(info), n, arr, len(reads)))
    if work is None:
        work = _work(need, inp.device)
    _check_work(work, inp.device, need)
    rc = lib().hc_seg_decompress_ranges_dev(_dp(inp), n, ctypes.byref(info), arr, len(reads), _dp(out), cap,
                                            _dp(out_len), _dp(status),
                                            ctypes.c_void_p(None) if bad_segment is None else _dp(bad_segment),
                                            _dp(work), work.numel(), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_seg_decompress_ranges_dev failed: {rc}")
    return work


def seg_append_plan(info, in_len, add_len):
    """hc_seg_append_plan (host only, no device): (status, the result's SegInfo or None, the first
    coded segment K, the decoded segments: 0 or 1) of add_len bytes appended to a container"""
    new = SegInfo()
    k = ctypes.c_uint64(0)
    dec = ctypes.c_uint64(0)
    st = lib().hc_seg_append_plan(ctypes.byref(info) if info is not None else None, in_len, add_len, ctypes.byref(new),
                                  ctypes.byref(k), ctypes.byref(dec))
    return st, (new if st == 0 else None), k.value, dec.value


def seg_append_bound(info, in_len, add_len):
    """hc_seg_append_bound: an output capacity that always suffices (0: the call refuses the arguments)"""
    return int(lib().hc_seg_append_bound(ctypes.byref(info) if info is not None else None, in_len, add_len))


def seg_append_work_bound(info, in_len, add_len):
    """hc_seg_append_work_bound: the device call's workspace (0: refused; 16: an info that fails)"""
    return int(lib().hc_seg_append_work_bound(ctypes.byref(info) if info is not None else None, in_len, add_len))


def seg_append(data, add, full=False, cap=None):
    """hc_seg_append: (status, the container of the raw bytes of `data` followed by `add`); full:
    (status, bytes, out_len, bad_segment). cap: the output capacity (default: hc_seg_append_bound)."""
    b, p = _buf(data)
    ab, ap = _buf(add)
    if cap is None:
        st, info = seg_info(b)
        cap = seg_append_bound(info, len(b), len(ab)) if st == 0 else 0
    out = ctypes.create_string_buffer(max(int(cap), 1))
    n = ctypes.c_uint64(0)
    bad = ctypes.c_uint64(NO_SEGMENT)
    st = lib().hc_seg_append(p, len(b), ap, len(ab), ctypes.cast(out, ctypes.c_void_p), cap, ctypes.byref(n),
                             ctypes.byref(bad))
    got = out.raw[:n.value] if st == 0 else b""
    return (st, got, n.value, bad.value) if full else (st, got)


def seg_append_dev(inp, add, out, out_len, status, bad_segment=None, info=None, stream=None, work=None, in_len=None,
                   out_cap=None, add_len=None):
    """hc_seg_append_dev on CUDA tensors: the container in inp[:in_len] with add[:add_len] (a uint8
    tensor at any alignment) appended to its raw bytes, into `out` (capacity out_cap, default all of
    it). info as for seg_decompress_dev. Arguments that the call refuses raise. Returns the workspace."""
    _check_seg(inp, out, out_len, status, bad_segment)
    import torch
    if not isinstance(add, torch.Tensor) or add.dtype != torch.uint8 or not add.is_contiguous() \
            or add.device != inp.device:
        raise TypeError("add: expected a contiguous uint8 tensor on the input's device")
    n = inp.numel() if in_len is None else int(in_len)
    if n > inp.numel():
        raise ValueError(f"in_len {n} exceeds the {inp.numel()}-byte input tensor")
    cap = out.numel() if out_cap is None else int(out_cap)
    if cap > out.numel():
        raise ValueError(f"out_cap {cap} exceeds the {out.numel()}-byte output tensor")
    m = add.numel() if add_len is None else int(add_len)
    if m > add.numel():
        raise ValueError(f"add_len {m} exceeds the {add.numel()}-byte tensor")
    if info is None:
        head, p = _buf(inp[:min(n, 48)].cpu().numpy().tobytes())
        info = SegInfo()  # stays all zero when the header does not parse: the call rejects it
        lib().hc_seg_info(p, n, ctypes.byref(info))
    need = int(lib().hc_seg_append_work_bound(ctypes.byref(info), n, m))
    if work is None:
        work = _work(need, inp.device)
    _check_work(work, inp.device, need)
    rc = lib().hc_seg_append_dev(_dp(inp), n, ctypes.byref(info), _dp(add) if m else ctypes.c_void_p(None), m,
                                 _dp(out), cap, _dp(out_len), _dp(status),
                                 ctypes.c_void_p(None) if bad_segment is None else _dp(bad_segment),
                                 _dp(work), work.numel(), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_seg_append_dev failed: {rc}")
    return work


def _check_seg_batch(inp, out, n, out_lens, status, bad_segments):
    """the tensor checks of _check_seg for the batched calls (one result per item)"""
    import torch
    spec = [("in", inp, torch.uint8, None), ("out", out, torch.uint8, None), ("out_lens", out_lens, torch.int64, n),
            ("status", status, torch.int32, n)]
    if bad_segments is not None:
        spec.append(("bad_segments", bad_segments, torch.int64, n))
    dev = inp.device if isinstance(inp, torch.Tensor) else None
    for name, t, dt, numel in spec:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch tensor")
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{name}: expected a CUDA tensor on {dev}, got {t.device}")
        if t.dtype != dt:
            raise TypeError(f"{name}: expected {dt}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
        if numel is not None and t.numel() != numel:
            raise ValueError(f"{name}: {t.numel()} entries for {n} items")


def seg_enc_items(items):
    """a ctypes array of SegEncItem from (in_off, in_len, width, out_off, out_cap) tuples"""
    return (SegEncItem * max(len(items), 1))(*[SegEncItem(*[int(v) for v in it]) for it in items])


def seg_dec_items(items):
    """a ctypes array of SegDecItem from (in_off, in_len, SegInfo, offset, length, out_off, out_cap)
    tuples; a None info stays all zero, which the call answers with HC_ERR_SEG_HEADER"""
    arr = (SegDecItem * max(len(items), 1))()
    for a, (in_off, in_len, info, offset, length, out_off, out_cap) in zip(arr, items):
        a.in_off, a.in_len, a.offset, a.length, a.out_off, a.out_cap = in_off, in_len, offset, length, out_off, out_cap
        if info is not None:
            a.info = info
    return arr


def seg_compress_batch_work_bound(items, use_diff=False, use_adapt=False, seg_bytes=0, check=False):
    """hc_seg_compress_batch_work_bound of item tuples (seg_enc_items); 0: the call refuses them"""
    return int(lib().hc_seg_compress_batch_work_bound(seg_enc_items(items), len(items),
                                                      _seg_flags(use_diff, use_adapt, check), seg_bytes))


def seg_decompress_batch_work_bound(items):
    """hc_seg_decompress_batch_work_bound of item tuples (seg_dec_items)"""
    return int(lib().hc_seg_decompress_batch_work_bound(seg_dec_items(items), len(items)))


def seg_compress_batch_dev(inp, out, items, out_lens, status, use_diff=False, use_adapt=False, seg_bytes=0,
                           check=False, stream=None, work=None):
    """hc_seg_compress_batch_dev on CUDA tensors: item i, an (in_off, in_len, width, out_off,
    out_cap) tuple, codes inp[in_off:+in_len] into one container at out[out_off:+out_cap];
    out_lens (int64) and status (int32) hold one device result per item, asynchronous on
    `stream`. The workspace is allocated here unless given. Returns it."""
    n = len(items)
    _check_seg_batch(inp, out, n, out_lens, status, None)
    flags = _seg_flags(use_diff, use_adapt, check)
    arr = seg_enc_items(items)
    need = int(lib().hc_seg_compress_batch_work_bound(arr, n, flags, seg_bytes))
    if work is None:
        work = _work(need, inp.device)
    rc = lib().hc_seg_compress_batch_dev(_dp(inp), _dp(out), arr, n, flags, seg_bytes, _dp(out_lens), _dp(status),
                                         _dp(work), work.numel(), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_seg_compress_batch_dev failed: {rc}")
    return work


def seg_decompress_batch_dev(inp, out, items, out_lens, status, bad_segments=None, stream=None, work=None):
    """hc_seg_decompress_batch_dev on CUDA tensors: item i, an (in_off, in_len, SegInfo, offset,
    length, out_off, out_cap) tuple, reads raw bytes [offset, offset + length) of the container
    at inp[in_off:+in_len] (0, HC_SEG_WHOLE: all of it) into out[out_off:+out_cap]. One device
    result per item in out_lens, status and bad_segments. Returns the workspace."""
    n = len(items)
    _check_seg_batch(inp, out, n, out_lens, status, bad_segments)
    arr = seg_dec_items(items)
    need = int(lib().hc_seg_decompress_batch_work_bound(arr, n))
    if work is None:
        work = _work(need, inp.device)
    rc = lib().hc_seg_decompress_batch_dev(_dp(inp), _dp(out), arr, n, _dp(out_lens), _dp(status),
                                           ctypes.c_void_p(None) if bad_segments is None else _dp(bad_segments),
                                           _dp(work), work.numel(), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_seg_decompress_batch_dev failed: {rc}")
    return work


def seg_compress_host_batch(blobs, use_diff=False, use_adapt=False, widths=None, seg_bytes=0, check=False, caps=None):
    """hc_seg_compress_host_batch on host byte strings: (statuses, containers, out_lens); widths:
    one per blob (default 512 each). caps: the output capacities (default: hc_seg_compress_bound2)."""
    flags = _seg_flags(use_diff, use_adapt, check)
    widths = [512] * len(blobs) if widths is None else widths
    if caps is None:
        caps = [lib().hc_seg_compress_bound2(len(b), seg_bytes if seg_bytes % 16 == 0 else 0, flags, w)
                for b, w in zip(blobs, widths)]
    w = (ctypes.c_uint64 * max(len(blobs), 1))(*[int(x) for x in widths])
    L = lib()

    def fn(ins, lens, n, outs, ocaps, olens, st):
        return L.hc_seg_compress_host_batch(ins, lens, ctypes.cast(w, ctypes.c_void_p), n, flags, seg_bytes, outs,
                                            ocaps, olens, st)
    return _host_batch(fn, blobs, caps)


def seg_decompress_host_batch(blobs, ranges=None, caps=None):
    """hc_seg_decompress_host_batch on host byte strings: (statuses, decoded, out_lens,
    bad_segments). ranges: None (every container whole) or one (offset, length) per blob; caps: the
    output capacities (default: the range's length, or the header's raw_len)."""
    n = len(blobs)
    if caps is None:
        caps = []
        for k, b in enumerate(blobs):
            if ranges is not None and tuple(ranges[k]) != (0, HC_SEG_WHOLE):
                caps.append(ranges[k][1])
            else:
                st, info = seg_info(b)
                caps.append(info.raw_len if st == 0 else 0)
    offs = lens = ctypes.c_void_p(None)
    if ranges is not None:
        o = (ctypes.c_uint64 * max(n, 1))(*[int(r[0]) for r in ranges])
        m = (ctypes.c_uint64 * max(n, 1))(*[int(r[1]) for r in ranges])
        offs, lens = ctypes.cast(o, ctypes.c_void_p), ctypes.cast(m, ctypes.c_void_p)
    bad = (ctypes.c_uint64 * max(n, 1))()
    L = lib()

    def fn(ins, ilens, n_items, outs, ocaps, olens, st):
        return L.hc_seg_decompress_host_batch(ins, ilens, offs, lens, n_items, outs, ocaps, olens, st,
                                              ctypes.cast(bad, ctypes.c_void_p))
    sts, res, olens = _host_batch(fn, blobs, caps)
    return sts, res, olens, [bad[i] for i in range(n)]


def crc32_batch(inp, in_offs, lens, crc, stream=None):
    """hc_crc32_batch on CUDA tensors: crc[i] (int32 or uint32 storage, one per range) =
    zlib.crc32(inp[in_offs[i]:+lens[i]]); any alignment, any length, asynchronous on `stream`."""
    import torch
    n = in_offs.numel()
    for name, t, dts in (("in", inp, (torch.uint8,)), ("in_offs", in_offs, (torch.int64,)), ("lens", lens, (torch.int64,)),
                         ("crc", crc, (torch.int32, getattr(torch, "uint32", torch.int32)))):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == inp.device and t.dtype in dts
                and t.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous {dts[0]} CUDA tensor on {inp.device}")
    if lens.numel() != n or crc.numel() != n:
        raise ValueError("in_offs, lens and crc must have one entry per range")
    rc = lib().hc_crc32_batch(_dp(inp), _dp(in_offs), _dp(lens), n, _dp(crc), _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_crc32_batch failed: {rc}")


def pack_batch(inp, in_offs, lens, out, out_offs, stream=None):
    """hc_pack_batch on CUDA tensors: out[out_offs[i]:+lens[i]] = inp[in_offs[i]:+lens[i]]."""
    import torch
    n = in_offs.numel()
    for name, t, dt in (("in", inp, torch.uint8), ("in_offs", in_offs, torch.int64), ("lens", lens, torch.int64),
                        ("out", out, torch.uint8), ("out_offs", out_offs, torch.int64)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == inp.device and t.dtype == dt
                and t.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous {dt} CUDA tensor on {inp.device}")
    if lens.numel() != n or out_offs.numel() != n:
        raise ValueError("in_offs, lens and out_offs must have one entry per range")
    rc = lib().hc_pack_batch(_dp(inp), _dp(in_offs), _dp(lens), n, _dp(out), _dp(out_offs),
                             _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_pack_batch failed: {rc}")


def _host_batch(fn, blobs, caps, *extra):
    """blobs in host memory -> (statuses, outputs) through a host-batch entry point"""
    n = len(blobs)
    keep = [bytes(b) for b in blobs]
    ins = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) if b else None
                                          for b in keep])
    lens = (ctypes.c_uint64 * max(n, 1))(*[len(b) for b in keep])
    outs_buf = [ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(o, ctypes.c_void_p) for o in outs_buf])
    ocaps = (ctypes.c_uint64 * max(n, 1))(*[int(c) for c in caps])
    olens = (ctypes.c_uint64 * max(n, 1))()
    st = (ctypes.c_int32 * max(n, 1))()
    rc = fn(ctypes.cast(ins, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p), n, *extra,
            ctypes.cast(outs, ctypes.c_void_p), ctypes.cast(ocaps, ctypes.c_void_p),
            ctypes.cast(olens, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p))
    if rc:
        raise HCodecError(f"host batch failed: {rc}")
    res = [outs_buf[i].raw[:olens[i]] if st[i] == 0 else b"" for i in range(n)]
    return [st[i] for i in range(n)], res, [olens[i] for i in range(n)]


def compress_host_batch(blobs, use_diff=False, caps=None):
    """hc_compress_host_batch on host byte strings: (statuses, encoded, out_lens)."""
    caps = caps if caps is not None else [compress_bound(len(b)) for b in blobs]
    return _host_batch(lib().hc_compress_host_batch, blobs, caps, HC_FLAG_DIFF if use_diff else 0)


def compress_adapt_host_batch(blobs, widths, use_diff=False, caps=None):
    """hc_compress_adapt_host_batch on host byte strings (-a, one matrix of widths[i] per blob):
    (statuses, encoded, out_lens)."""
    caps = caps if caps is not None else [compress_bound(len(b), True) for b in blobs]
    w = (ctypes.c_uint64 * max(len(blobs), 1))(*[int(x) for x in widths])
    L = lib()

    def fn(ins, lens, n, outs, ocaps, olens, st):
        return L.hc_compress_adapt_host_batch(ins, lens, ctypes.cast(w, ctypes.c_void_p), n,
                                              HC_FLAG_DIFF if use_diff else 0, outs, ocaps, olens, st)
    return _host_batch(fn, blobs, caps)


def decompress_host_batch(blobs, caps):
    """hc_decompress_host_batch on host byte strings: (statuses, decoded, out_lens)."""
    return _host_batch(lib().hc_decompress_host_batch, blobs, caps)


def synth_batch(kind, k0, n_streams, width, height, out, stride, stream=None):
    """hc_synth_batch: SURVEY.md Appendix D inputs generated in device memory."""
    rc = lib().hc_synth_batch(SYNTH.get(kind, kind), k0, n_streams, width, height, _dp(out),
                              stride, _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_synth_batch failed: {rc}")


def debug_set_window(nbytes):
    """Test hook (debug build only, use_debug_build): the FGK kernels reach each stream through buffer
    windows that slide every `nbytes` (default 1 GiB); a small window makes ordinary streams
    cross many window edges. Affects every later launch in this process."""
    f = _dbg().hc_debug_set_window
    f.argtypes = [ctypes.c_uint32]
    rc = f(int(nbytes))
    if rc:
        raise HCodecError(f"hc_debug_set_window failed: {rc}")


def debug_set_min_tree(kind):
    """Test hook (debug build only, use_debug_build): the smallest FGK tree layout every later launch
    in this process may use (0 narrow, 1 wide, 2 huge: 64-bit weights), so that small streams
    exercise the kernels otherwise reserved for streams of > 2^22 - 2 / >= 2^32 - 1 symbols."""
    f = _dbg().hc_debug_set_min_tree
    f.argtypes = [ctypes.c_uint32]
    rc = f(int(kind))
    if rc:
        raise HCodecError(f"hc_debug_set_min_tree failed: {rc}")


def debug_set_enc_tab(mode):
    """Test hook (debug build only, use_debug_build): how the encoder finds a symbol's code for
    narrow / wide streams: 0 per stream from a sample of its alphabet (the default), 1 the path
    cache for every stream, 2 the level tables for every stream, 3 the small-alphabet kernel for
    every narrow stream."""
    f = _dbg().hc_debug_set_enc_tab
    f.argtypes = [ctypes.c_uint32]
    rc = f(int(mode))
    if rc:
        raise HCodecError(f"hc_debug_set_enc_tab failed: {rc}")


def debug_set_dec_small(mode):
    """Test hook (debug build only, use_debug_build): which decoder launch takes a narrow stream:
    0 by its payload rate (under 2.5 bits per symbol: the small-alphabet launch; the default), 1
    the small-alphabet launch for every one, 2 the regular launch for every one."""
    f = _dbg().hc_debug_set_dec_small
    f.argtypes = [ctypes.c_uint32]
    rc = f(int(mode))
    if rc:
        raise HCodecError(f"hc_debug_set_dec_small failed: {rc}")


def debug_set_dec_pack(max_codes):
    """Test hook (debug build only, use_debug_build): the most codes one batch step of the FGK
    decoder takes (Dec::decode_batch): 1, 7, or 16 (the build's own cap; any other value). A device
    variable, like debug_set_window's: it holds for later launches on the current device only."""
    f = _dbg().hc_debug_set_dec_pack
    f.argtypes = [ctypes.c_uint32]
    rc = f(int(max_codes))
    if rc:
        raise HCodecError(f"hc_debug_set_dec_pack failed: {rc}")


def debug_set_enc_pack(max_symbols):
    """Test hook (debug build only, use_debug_build): the most symbols one regular batch step of the
    FGK encoder takes (code_all_batch): 1, 7, or 16 (the build's own cap; any other value). A device
    variable, like debug_set_dec_pack's: it holds for later launches on the current device only."""
    f = _dbg().hc_debug_set_enc_pack
    f.argtypes = [ctypes.c_uint32]
    rc = f(int(max_symbols))
    if rc:
        raise HCodecError(f"hc_debug_set_enc_pack failed: {rc}")


def debug_enc_votes(inp, in_offs, in_lens, use_diff, low_occ, status, stream=None):
    """Test hook (debug build only, use_debug_build): the encoder's per-stream mode vote alone
    (enc_mode_kernel) into status: -0x7A1 the path cache, -0x7A0 the level tables. low_occ: the
    batch fits table mode's residency (what the launcher passes for <= 24 streams per CU)."""
    n = _check_batch(inp, in_offs, in_lens, inp, in_offs, in_lens, in_lens, status)
    f = _dbg().hc_debug_enc_votes
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 2
    rc = f(_dp(inp), _dp(in_offs), _dp(in_lens), n, HC_FLAG_DIFF if use_diff else 0, 1 if low_occ else 0, _dp(status),
           _stream_handle(stream))
    if rc:
        raise HCodecError(f"hc_debug_enc_votes failed: {rc}")


def debug_set_par_min(symbols):
    """Test hook (debug build only, use_debug_build): adaptive streams of at least `symbols` block
    symbols find their block boundaries by the parallel pass (default 2^20; 0: every stream)."""
    f = _dbg().hc_debug_set_par_min
    f.argtypes = [ctypes.c_uint64]
    rc = f(int(symbols))
    if rc:
        raise HCodecError(f"hc_debug_set_par_min failed: {rc}")


def debug_set_par_skew(nbytes):
    """Test hook (debug build only, use_debug_build): every odd chunk of the parallel block-boundary
    pass walks from its predicted entry shifted by `nbytes` output bytes (0: off), forcing par_fix's
    re-runs and its repair of the block starts a wrong walk wrote."""
    f = _dbg().hc_debug_set_par_skew
    f.argtypes = [ctypes.c_uint64]
    rc = f(int(nbytes))
    if rc:
        raise HCodecError(f"hc_debug_set_par_skew failed: {rc}")


def debug_stage_clock(on):
    """Diagnostic (debug build only, use_debug_build): when on, the batched adaptive calls of
    this thread record a HIP event after each stage; debug_stage_times() reads the last call's."""
    f = _dbg().hc_debug_stage_clock
    f.argtypes = [ctypes.c_int]
    f(1 if on else 0)


def debug_stage_times():
    """[(stage, ms), ...] of the last batched adaptive call (waits for it); needs the clock on"""
    f = _dbg().hc_debug_stage_times
    f.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    names = ctypes.create_string_buffer(1024)
    ms = (ctypes.c_float * 32)()
    n = f(names, 1024, ms, 32)
    if n < 0:
        raise HCodecError("hc_debug_stage_times failed (clock off?)")
    return list(zip(names.value.decode().split("\n")[:n], [float(ms[k]) for k in range(n)]))


def compress_bound(n, use_adapt=False):
    return int(lib().hc_compress_bound(n, int(bool(use_adapt))))


def device_ok():
    return bool(lib().hc_device_ok())


def device_info():
    buf = ctypes.create_string_buffer(512)
    lib().hc_device_info(buf, 512)
    return buf.value.decode()


def version():
    return lib().hc_version().decode()


def header_symbols():
    """Every function name declared in include/*.h (the exported surface)."""
    import re
    names = []
    for fn in sorted(os.listdir(INCLUDE_DIR)):
        if fn.endswith(".h"):
            txt = open(os.path.join(INCLUDE_DIR, fn)).read()
            txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
            names += re.findall(r"\b(hc_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(names))
