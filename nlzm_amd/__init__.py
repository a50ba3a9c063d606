"""nlzm_amd -- MI355X (gfx950) implementation of NLZM 1.03's compress-side hot path.

The product is the C-ABI shared library ``libnlzm_hip.so`` (include/nlzm_hip.h) and the
``nlzm`` command line built from ``nlzm_amd/csrc``.  This module is the thin ctypes
binding the tests and ``bench.py`` use; it adds no algorithmic code and has no CPU
fallback: every call below fails loudly if the library or a gfx950 device is missing.
The signatures are the table in ``_abi.py``; the sidecar index reader is ``index.py``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

# block mode keeps several persistent launches in flight; the HIP runtime's default of 4 hardware queues would serialise
# them (only effective if the runtime has not started yet)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

from ._abi import ABI_SYMBOLS, Stats, Timing, bind                    # noqa: E402,F401  (re-exported)
from .index import read_index, read_index_typed                        # noqa: E402,F401  (re-exported)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NLZM_LIB", os.path.join(_HERE, "libnlzm_hip.so"))     # override: diagnostic builds only
CLI_PATH = os.path.join(_HERE, "nlzm")

DECODE_MORE = 1          # NLZM_HIP_DECODE_MORE
TO_THE_END = (1 << 64) - 1


class NlzmError(RuntimeError):
    pass


def build(force: bool = False) -> None:
    """Compile the gfx950 library and the CLI in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j8", "all"], capture_output=True, text=True)
    if r.returncode != 0:
        raise NlzmError("building libnlzm_hip.so failed:\n" + r.stdout + r.stderr)


_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree library (no device needed just to load it) and give it the signatures of _abi.TABLE."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NlzmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)")
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def _chk(rc: int) -> None:
    if rc != 0:
        raise NlzmError(f"nlzm_hip error {rc}: {load_library().nlzm_hip_last_error().decode()}")


# ---- marshalling: what every function below hands to the library, and takes back

def _bytes_in(data) -> np.ndarray:
    return np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)


def _ptr(a: np.ndarray):
    """the array's address, NULL when it is empty"""
    return a.ctypes.data if a.size else None


def _arr(ctype, values, slots: int = 0):
    """a ctypes array of the integers `values`, `slots` entries long at least; None stays None (NULL)"""
    if values is None:
        return None
    values = [int(v) for v in values]
    return (ctype * max(slots, len(values)))(*values)


def _ranges(ranges, slots: int = 0):
    """(k, off[], len[]) of a list of (offset, length)"""
    return len(ranges), _arr(C.c_uint64, [o for o, _ in ranges], slots), _arr(C.c_uint64, [l for _, l in ranges], slots)


def _elems(elems, slots: int = 0):
    """element sizes as bytes; one that does not fit a byte goes as 0, which the library refuses by the range's name"""
    return None if elems is None else _arr(C.c_uint8, [int(e) if 0 <= int(e) < 256 else 0 for e in elems], slots)


def _crcs(crcs):
    return None if crcs is None else _arr(C.c_uint32, [int(c) & 0xFFFFFFFF for c in crcs])


def _one_per_block(k: int, **lists) -> None:
    for name, v in lists.items():
        if v is not None and len(v) != k:
            raise ValueError(f"{name}: one entry per block")


def _cut(buf, lens, total=None, take=lambda piece: piece.tobytes()) -> list:
    """buf cut into one piece per length, back to back; total: what the lengths must come to"""
    out, pos = [], 0
    for n in lens:
        out.append(take(buf[pos: pos + int(n)]))
        pos += int(n)
    assert total is None or pos == total
    return out


def _with_dedup(dedup: bool, call):
    """call() with option "dedup_ranges" set for its duration when dedup is true, the option as it stood afterwards"""
    if not dedup:
        return call()
    was = counter("dedup_ranges")        # (the option as it stands)
    set_option("dedup_ranges", 1)
    try:
        return call()
    finally:
        set_option("dedup_ranges", was)


# ---- the entry points

def init(device: int = 0) -> None:
    _chk(load_library().nlzm_hip_init(device))


def shutdown() -> None:
    load_library().nlzm_hip_shutdown()


def set_option(key: str, value: int) -> None:
    _chk(load_library().nlzm_hip_set_option(key.encode(), int(value)))


def geometry(flen: int, hist_bits: int) -> dict:
    lib = load_library()
    v = [C.c_uint32() for _ in range(4)]
    lib.nlzm_hip_geometry(flen, hist_bits, *[C.byref(x) for x in v])
    return dict(zip(("hist_bits", "frame_bits", "chunk_size", "feed_size"), (int(x.value) for x in v)))


def compress(data, hist_bits: int = 22) -> bytes:
    """encode_file replacement on host buffers (NLZM.cpp:1711); returns the whole stream."""
    lib = load_library()
    src = _bytes_in(data)
    n = int(src.size)
    cap = int(lib.nlzm_hip_compress_bound(n))
    dst = np.empty(cap, dtype=np.uint8)
    out_len = C.c_uint64(0)
    _chk(lib.nlzm_hip_compress(_ptr(src), n, hist_bits, dst.ctypes.data, cap, C.byref(out_len)))
    return dst[: out_len.value].tobytes()


def compress_blocks(data, nblocks: int, hist_bits: int = 22) -> list[bytes]:
    """k independent streams (shard.block_range gives the byte ranges), 1 to 65536: in flight on the one GPU all at once while a launch holds
    them (64 on an MI355X), more of them in sets one after another (option "container_set_blocks"; counter "container_sets"); the reference
    equivalent is encode_file (NLZM.cpp:1711) run on each range."""
    lib = load_library()
    src = _bytes_in(data)
    n = int(src.size)
    if not 1 <= nblocks <= 65536:
        raise ValueError("nblocks: 1 to 65536")
    cap = int(lib.nlzm_hip_compress_blocks_bound(n, nblocks))       # (a guaranteed bound; the pages the streams do not reach are never touched)
    dst = np.empty(cap, dtype=np.uint8)
    lens = (C.c_uint64 * nblocks)()
    out_len = C.c_uint64(0)
    _chk(lib.nlzm_hip_compress_blocks(_ptr(src), n, nblocks, hist_bits, dst.ctypes.data, cap, lens, C.byref(out_len)))
    return _cut(dst, lens, out_len.value)


def equal_ranges(data, ranges, fingerprints=None) -> list[int]:
    """first_of for the (offset, length) ranges of `data`, found on the device (nlzm_hip_equal_ranges): first_of[i] is the smallest j <= i whose
    range holds the same bytes as range i.  Exact: fingerprints group the ranges, byte compares decide.  fingerprints: a list that receives every
    range's 64-bit fingerprint (the rule: tests/dedup_model.py)."""
    lib = load_library()
    src = _bytes_in(data)
    if not 1 <= len(ranges) <= 65536:
        raise ValueError("ranges: 1 to 65536")
    k, off, ln = _ranges(ranges)
    first, fp = (C.c_uint32 * k)(), (C.c_uint64 * k)()
    _chk(lib.nlzm_hip_equal_ranges(_ptr(src), int(src.size), k, off, ln, first, fp))
    if fingerprints is not None:
        fingerprints[:] = [int(x) for x in fp]
    return [int(x) for x in first]


def _compress_ranges(entry, src, ranges, extra: tuple, hist_bits: int, dedup: bool) -> list[bytes]:
    """what compress_ranges and compress_typed share: `entry` is the library's function, `extra` what it takes between the lengths and the window"""
    k, off, ln = _ranges(ranges)
    cap = int(load_library().nlzm_hip_compress_ranges_bound(k, ln))
    dst = np.empty(max(1, cap), dtype=np.uint8)
    lens = (C.c_uint64 * k)()
    out_len = C.c_uint64(0)
    _with_dedup(dedup, lambda: _chk(entry(_ptr(src), int(src.size), k, off, ln, *extra, hist_bits, dst.ctypes.data, cap, lens, C.byref(out_len))))
    return _cut(dst, lens, out_len.value)


def compress_ranges(data, ranges, hist_bits: int = 22, dedup: bool = False) -> list[bytes]:
    """One stream per (offset, length) range of `data`, all in one call: the ranges may be empty, overlap, repeat and come in any order; stream i
    is the reference's encode_file (NLZM.cpp:1711) run on data[off:off + length].  Up to a launch's capacity (64 on an MI355X) they are one block
    set, more of them run in sets of consecutive ranges (counter "container_sets").  dedup: option "dedup_ranges" for this call -- a range whose
    bytes an earlier one holds is not compressed again, its stream is a copy (the same bytes come back; the "dedup_*" counters say what was saved)."""
    if dedup:                # (the option is set before the arguments are looked at)
        return _with_dedup(True, lambda: compress_ranges(data, ranges, hist_bits))
    lib = load_library()
    src = _bytes_in(data)
    if not 1 <= len(ranges) <= 65536:
        raise ValueError("ranges: 1 to 65536")
    return _compress_ranges(lib.nlzm_hip_compress_ranges, src, ranges, (), hist_bits, False)


def planes(data, ranges, elems, inverse: bool = False) -> list[bytes]:
    """The byte planes of every (offset, length) range of `data` at its element size (1, 2, 4 or 8), made on the device in one launch
    (nlzm_hip_planes; the rule: tests/planes_model.py): byte j of every element goes to plane j, the tail bytes behind the last whole element stay.
    inverse: the filter undone.  The ranges may be empty, overlap and repeat; one result per range."""
    lib = load_library()
    src = _bytes_in(data)
    if not 1 <= len(ranges) <= 65536 or len(elems) != len(ranges):
        raise ValueError("ranges: 1 to 65536, one element size each")
    k, off, ln = _ranges(ranges)
    lens = [int(l) for _, l in ranges]
    ok = all(0 <= l < 1 << 48 for l in lens)       # (a length that cannot be: the library names the range, and nothing is written)
    at, total = [], 0
    for l in lens:
        at.append(total)
        total += l if ok else 0
    dst = np.empty(max(1, total), dtype=np.uint8)
    _chk(lib.nlzm_hip_planes(_ptr(src), int(src.size), dst.ctypes.data, total, k, off, _arr(C.c_uint64, at), ln, _elems(elems), 1 if inverse else 0))
    return [dst[a: a + l].tobytes() for a, l in zip(at, lens)]


def compress_typed(data, ranges, elems, hist_bits: int = 22, dedup: bool = False) -> list[bytes]:
    """compress_ranges with an element size (1, 2, 4 or 8) per range: stream i is the reference's encode_file run on the byte planes of range i
    (nlzm_hip_compress_ranges_typed), which the reference decompressor reads and planes(..., inverse=True) -- one line of numpy -- undoes.
    elems None: compress_ranges itself."""
    lib = load_library()
    src = _bytes_in(data)
    if not 1 <= len(ranges) <= 65536 or (elems is not None and len(elems) != len(ranges)):
        raise ValueError("ranges: 1 to 65536, one element size each")
    return _compress_ranges(lib.nlzm_hip_compress_ranges_typed, src, ranges, (_elems(elems),), hist_bits, dedup)


def decompress_typed(blob, block_lens, raw_lens, elems) -> list[bytes]:
    """The blocks of a typed container (the streams of compress_typed, joined) decoded on the device with the filter undone
    (nlzm_hip_decompress_blocks_typed): one result per block.  block_lens / raw_lens may be None (the hop over the frame headers; a size pass)."""
    lib = load_library()
    src = _bytes_in(blob)
    k = len(elems)
    _one_per_block(k, block_lens=block_lens, raw_lens=raw_lens)
    blen, raw, el = _arr(C.c_uint64, block_lens), _arr(C.c_uint64, raw_lens, 1), _elems(elems, 1)
    got, total = (C.c_uint64 * max(1, k))(), C.c_uint64(0)
    if raw is None:
        _chk(lib.nlzm_hip_decompress_blocks_typed(src.ctypes.data, src.size, k, blen, None, el, None, 0, got, C.byref(total)))
        raw = got
    cap = sum(int(raw[i]) for i in range(k))
    dst = np.empty(max(1, cap), dtype=np.uint8)
    _chk(lib.nlzm_hip_decompress_blocks_typed(src.ctypes.data, src.size, k, blen, raw, el, dst.ctypes.data, cap, got, C.byref(total)))
    return _cut(dst, got[:k], total.value)


def plane_costs(data, ranges, hist: bool = False):
    """(C_1, C_2, C_4, C_8) of every (offset, length) range of `data`, counted on the device in one launch (nlzm_hip_plane_costs; the rule:
    tests/elem_model.py): what the range's byte planes at element size 1, 2, 4 and 8 would cost an order-0 coder, in 2^-16 bits, model included.
    hist: also the counts they were made from, an array of shape (k, 8, 256) -- H[c][v] of every range."""
    lib = load_library()
    src = _bytes_in(data)
    if not 1 <= len(ranges) <= 65536:
        raise ValueError("ranges: 1 to 65536")
    k, off, ln = _ranges(ranges)
    cost = (C.c_uint64 * (4 * k))()
    h = np.zeros((k, 8, 256), dtype=np.uint64) if hist else None
    _chk(lib.nlzm_hip_plane_costs(_ptr(src), int(src.size), k, off, ln, cost, None if h is None else h.ctypes.data_as(C.POINTER(C.c_uint64))))
    costs = [tuple(int(cost[4 * i + j]) for j in range(4)) for i in range(k)]
    return (costs, h) if hist else costs


def choose_elem(costs, length: int) -> int:
    """The element size (1, 2, 4 or 8) for a range of `length` bytes with the costs (C_1, C_2, C_4, C_8) (nlzm_hip_choose_elem); needs no device."""
    if len(costs) != 4:
        raise ValueError("costs: C_1, C_2, C_4, C_8")
    return int(load_library().nlzm_hip_choose_elem(_arr(C.c_uint64, costs), int(length)))


def choose_elems(data, ranges) -> list[int]:
    """The element size chosen for every (offset, length) range of `data`: plane_costs and choose_elem in one call (nlzm_hip_choose_elems)."""
    lib = load_library()
    src = _bytes_in(data)
    if not 1 <= len(ranges) <= 65536:
        raise ValueError("ranges: 1 to 65536")
    k, off, ln = _ranges(ranges)
    el = (C.c_uint8 * k)()
    _chk(lib.nlzm_hip_choose_elems(_ptr(src), int(src.size), k, off, ln, el))
    return [int(e) for e in el]


def compress_auto(data, ranges, hist_bits: int = 22, dedup: bool = False):
    """compress_typed with the element sizes chosen on the device from the ranges' bytes (nlzm_hip_compress_ranges_auto): (streams, elems), and
    decompress_typed reads the streams with elems."""
    lib = load_library()
    src = _bytes_in(data)
    if not 1 <= len(ranges) <= 65536:
        raise ValueError("ranges: 1 to 65536")
    el = (C.c_uint8 * len(ranges))()
    streams = _compress_ranges(lib.nlzm_hip_compress_ranges_auto, src, ranges, (el,), hist_bits, dedup)
    return streams, [int(e) for e in el]


def _tensor_elem(t) -> int:
    return t.element_size() if t.element_size() in (2, 4, 8) else 1


def compress_tensors(tensors, hist_bits: int = 22, dedup: bool = False, auto: bool = False):
    """A list of torch tensors (any device, any dtype) as one block container in device memory, one block per tensor, filtered at the tensor's element
    size (1 when it is not 2, 4 or 8): the tensors are viewed as bytes and concatenated on the GPU, with the padding the compress path reads behind
    them, and nlzm_hip_compress_ranges_typed_dev runs on data_ptr().  auto: a tensor whose element size is 1 -- a uint8 tensor of packed records --
    is filtered at the size chosen from its bytes (nlzm_hip_choose_elems_dev); every other tensor keeps its dtype's.  Returns (container, meta): a
    device uint8 tensor and a list of (block_len, raw_len, elem, dtype, shape) per tensor -- what decompress_tensors takes."""
    import torch
    lib = load_library()
    k = len(tensors)
    if not 1 <= k <= 65536:
        raise ValueError("tensors: 1 to 65536")
    dev = torch.device("cuda", torch.cuda.current_device())
    flat = [t.detach().contiguous().reshape(-1).view(torch.uint8).to(dev) for t in tensors]
    lens = [int(f.numel()) for f in flat]
    data = torch.cat(flat + [torch.zeros(128, dtype=torch.uint8, device=dev)])
    at, n = [], 0
    for l in lens:
        at.append(n)
        n += l
    off, ln, el = _arr(C.c_uint64, at), _arr(C.c_uint64, lens), _arr(C.c_uint8, [_tensor_elem(t) for t in tensors])
    cap = int(lib.nlzm_hip_compress_ranges_bound(k, ln))
    out = torch.empty(max(1, cap), dtype=torch.uint8, device=dev)
    blen, got = (C.c_uint64 * k)(), C.c_uint64(0)
    torch.cuda.synchronize()
    bytewise = [i for i in range(k) if tensors[i].element_size() == 1] if auto else []
    if bytewise:
        chosen = (C.c_uint8 * len(bytewise))()
        _chk(lib.nlzm_hip_choose_elems_dev(data.data_ptr(), n, len(bytewise), _arr(C.c_uint64, [at[i] for i in bytewise]), _arr(C.c_uint64, [lens[i] for i in bytewise]), chosen))
        for i, e in zip(bytewise, chosen):
            el[i] = e
    _with_dedup(dedup, lambda: _chk(lib.nlzm_hip_compress_ranges_typed_dev(data.data_ptr(), n, k, off, ln, el, hist_bits, out.data_ptr(), cap, blen, C.byref(got))))
    meta = [(int(blen[i]), lens[i], int(el[i]), tensors[i].dtype, tuple(tensors[i].shape)) for i in range(k)]
    return out[: got.value].clone(), meta


def decompress_tensors(container, meta):
    """The inverse of compress_tensors: the tensors, on the container's device, bit for bit."""
    import torch
    lib = load_library()
    k = len(meta)
    if not 1 <= k <= 65536:
        raise ValueError("meta: 1 to 65536 entries")
    blen, raw, el = _arr(C.c_uint64, [m[0] for m in meta]), _arr(C.c_uint64, [m[1] for m in meta]), _arr(C.c_uint8, [m[2] for m in meta])
    total = sum(int(m[1]) for m in meta)
    src = container.contiguous()
    dst = torch.empty(max(1, total), dtype=torch.uint8, device=src.device)
    got = C.c_uint64(0)
    torch.cuda.synchronize()
    _chk(lib.nlzm_hip_decompress_blocks_typed_dev(src.data_ptr(), int(src.numel()), k, blen, raw, el, dst.data_ptr(), total, None, C.byref(got)))
    assert got.value == total
    pieces = _cut(dst, [m[1] for m in meta], take=lambda piece: piece.clone())
    return [p.view(m[3]).reshape(m[4]) for p, m in zip(pieces, meta)]


def cut_points(data, avg_bits: int, min_len=None, max_len=None) -> list[int]:
    """Content-defined cut points of `data`, found on the device (nlzm_hip_cut_points; the rule: tests/cut_model.py): ascending offsets inside
    (0, len(data)); blocks of 2^avg_bits bytes on average, min_len (default 2^(avg_bits - 2), 32 at least) to max_len (default 2^(avg_bits + 2))."""
    lib = load_library()
    src = _bytes_in(data)
    n = int(src.size)
    lo = max(32, 1 << max(0, avg_bits - 2)) if min_len is None else int(min_len)
    hi = max(lo, min(1 << 31, 1 << (avg_bits + 2))) if max_len is None else int(max_len)
    cap = min(n // max(lo, 1), 0xFFFFFFFF) if lo > 0 else 0
    cuts = (C.c_uint64 * max(1, cap))()
    got = C.c_uint32(0)
    _chk(lib.nlzm_hip_cut_points(_ptr(src), n, avg_bits, lo, hi, cuts, cap, C.byref(got)))
    return [int(cuts[i]) for i in range(got.value)]


def cut_ranges(n: int, cuts) -> list[tuple[int, int]]:
    """The (offset, length) blocks that the ascending cut points `cuts` make of n bytes: len(cuts) + 1 of them, back to back."""
    edges = [0] + [int(c) for c in cuts] + [int(n)]
    if any(b < a for a, b in zip(edges, edges[1:])):
        raise ValueError("cuts: ascending offsets within the input")
    return [(a, b - a) for a, b in zip(edges, edges[1:])]


def compress_fed(data, hist_bits: int = 22, piece: int = 1 << 20) -> bytes:
    """The streaming form of compress(): the input handed over `piece` bytes at a time (pinned staging, uploads overlapped
    with the launches), the stream taken back as its frames are finished (NLZM.cpp:1774-1778, :1853, :1870-1885)."""
    lib = load_library()
    src = _bytes_in(data)
    n = int(src.size)
    _chk(lib.nlzm_hip_feed_begin(n, hist_bits))
    buf = np.empty(1 << 20, dtype=np.uint8)
    got = C.c_uint64(0)
    out = []

    def drain():
        while True:
            _chk(lib.nlzm_hip_feed_output(buf.ctypes.data, buf.size, C.byref(got)))
            if not got.value:
                return
            out.append(buf[: got.value].tobytes())

    try:
        for lo in range(0, n, piece):
            m = min(piece, n - lo)
            _chk(lib.nlzm_hip_feed(src[lo:].ctypes.data, m))
            drain()
        _chk(lib.nlzm_hip_feed_finish())
        drain()
    finally:
        lib.nlzm_hip_feed_end()
    return b"".join(out)


def compress_blocks_multi(data, devices: list[int], blocks_per_dev: int, hist_bits: int = 22) -> list[bytes]:
    """len(devices) * blocks_per_dev independent streams, blocks_per_dev of them in flight on each listed GPU of this node
    (one host thread per GPU inside the library, no traffic between the GPUs but the final gather onto devices[0])."""
    lib = load_library()
    src = _bytes_in(data)
    n = int(src.size)
    nblocks = len(devices) * blocks_per_dev
    cap = int(lib.nlzm_hip_compress_bound(n)) + nblocks * (16 + 131072)
    dst = np.empty(cap, dtype=np.uint8)
    lens = (C.c_uint64 * nblocks)()
    out_len = C.c_uint64(0)
    devs = (C.c_int * len(devices))(*devices)
    _chk(lib.nlzm_hip_compress_blocks_multi(devs, len(devices), blocks_per_dev, _ptr(src), n, hist_bits,
                                            dst.ctypes.data, cap, lens, C.byref(out_len)))
    return _cut(dst, lens, out_len.value)


def decompress(stream) -> bytes:
    """decode_file replacement on host buffers (NLZM.cpp:1912): the stream is decoded on the device, one workgroup."""
    return b"".join(decompress_blocks(stream, 1))


def decompress_blocks(blob, nblocks: int) -> list[bytes]:
    """nblocks streams back to back (what compress_blocks returns, joined), decoded at once, one workgroup each."""
    lib = load_library()
    src = _bytes_in(blob)
    raw = (C.c_uint64 * nblocks)()
    total = C.c_uint64(0)
    _chk(lib.nlzm_hip_decompress_blocks(src.ctypes.data, src.size, nblocks, None, None, None, 0, raw, C.byref(total)))
    dst = np.empty(max(1, total.value), dtype=np.uint8)
    _chk(lib.nlzm_hip_decompress_blocks(src.ctypes.data, src.size, nblocks, None, raw, dst.ctypes.data, total.value, raw, C.byref(total)))
    return _cut(dst, raw)


class LengthMismatch(NlzmError):
    """verify: every byte of the original agrees, but the stream decodes to more bytes than the original has"""

    def __init__(self, decoded_len: int, n: int):
        super().__init__(f"the stream decodes to {decoded_len} bytes, the original has {n} (they agree up to there)")
        self.decoded_len, self.n = decoded_len, n


def verify_verdict(first: int, decoded_len: int, n: int) -> int:
    """What verify() answers for the library's (first_mismatch, decoded_len): n when equal (NLZM_HIP_VERIFY_EQUAL), an offset below n when a
    byte differs or the decode is shorter; a decode that is LONGER than an original it agrees with is not an offset below n and must not read
    as n either: it raises LengthMismatch."""
    if first == n and decoded_len == n:
        return n
    if first < n:
        return first
    raise LengthMismatch(decoded_len, n)


def verify(blob, data, nblocks: int = 1) -> int:
    """Decode `blob` (nblocks streams back to back) on the device and compare with `data`: the first differing offset, len(data) when equal
    (equal: the same bytes AND the same length -- see verify_verdict)."""
    lib = load_library()
    src, orig = _bytes_in(blob), _bytes_in(data)
    first, decoded = C.c_uint64(0), C.c_uint64(0)
    _chk(lib.nlzm_hip_verify(src.ctypes.data, src.size, nblocks, None, _ptr(orig), orig.size, C.byref(first), C.byref(decoded)))
    return verify_verdict(int(first.value), int(decoded.value), int(orig.size))


def crc32(data, seed: int = 0) -> int:
    """CRC32 (zlib.crc32's, the reference's crc32_calc) of `data`, uploaded and hashed on the device; `seed` chains calls as zlib's does."""
    lib = load_library()
    src = _bytes_in(data)
    out = C.c_uint32(0)
    _chk(lib.nlzm_hip_crc32(_ptr(src), src.size, seed & 0xFFFFFFFF, C.byref(out)))
    return int(out.value)


def crc32_ranges(data, ranges) -> list[int]:
    """The CRC32 of every (offset, length) range of `data`, all in one call on the device; the ranges may be empty and may overlap."""
    lib = load_library()
    src = _bytes_in(data)
    k, off, ln = _ranges(ranges, 1)
    out = (C.c_uint32 * max(1, k))()
    _chk(lib.nlzm_hip_crc32_ranges(_ptr(src), src.size, k, off, ln, out))
    return [int(out[i]) for i in range(k)]


def crc32_combine(a: int, b: int, len_b: int) -> int:
    """CRC32 of A + B from crc32(A), crc32(B) and len(B) (zlib's crc32_combine); needs no device."""
    return int(load_library().nlzm_hip_crc32_combine(a & 0xFFFFFFFF, b & 0xFFFFFFFF, len_b))


def check(blob, crcs, nblocks: int = 1, raw_lens=None) -> int:
    """Decode `blob` (nblocks streams back to back) on the device and compare every block's CRC32 -- and its length, where raw_lens gives
    them -- with what the caller holds; the original is not needed.  The first bad block, nblocks when none is."""
    lib = load_library()
    src = _bytes_in(blob)
    if len(crcs) != nblocks or (raw_lens is not None and len(raw_lens) != nblocks):
        raise ValueError("one CRC (and one length) per block")
    bad = C.c_uint32(0)
    _chk(lib.nlzm_hip_check(src.ctypes.data, src.size, nblocks, None, _arr(C.c_uint64, raw_lens), _crcs(crcs), C.byref(bad), None))
    return int(bad.value)


class CrcMismatch(NlzmError):
    """read_ranges: a block that was decoded in full does not hash to the CRC32 the caller holds for it"""

    def __init__(self, block: int):
        super().__init__(f"block {block} (counted from 0) does not decode to bytes with the CRC32 given for it")
        self.block = block


def read_ranges(blob, ranges, nblocks: int = 1, block_lens=None, raw_lens=None, crcs=None) -> list[bytes]:
    """The (offset, length) ranges of what `blob` (nblocks streams back to back) decodes to, all in one call on the device: only the blocks
    some range needs are decoded, each once and only as far as the furthest byte wanted of it.  With block_lens and raw_lens (read_index
    gives them) nothing else is touched or uploaded.  crcs: every block the call decoded in full is compared; CrcMismatch names the first
    that differs (blocks read in part cannot be checked)."""
    lib = load_library()
    src = _bytes_in(blob)
    _one_per_block(nblocks, block_lens=block_lens, raw_lens=raw_lens, crcs=crcs)
    k, off, ln = _ranges(ranges, 1)
    cap = sum(int(l) for _, l in ranges)
    dst = np.empty(max(1, cap), dtype=np.uint8)
    got, bad = C.c_uint64(0), C.c_uint32(nblocks)
    _chk(lib.nlzm_hip_read_ranges(src.ctypes.data, src.size, nblocks, _arr(C.c_uint64, block_lens), _arr(C.c_uint64, raw_lens), _crcs(crcs), k, off, ln,
                                  dst.ctypes.data, cap, C.byref(got), C.byref(bad)))
    if bad.value < nblocks:
        raise CrcMismatch(int(bad.value))
    return _cut(dst, [l for _, l in ranges], got.value)


def read_range(blob, off: int, length: int, nblocks: int = 1, block_lens=None, raw_lens=None, crcs=None) -> bytes:
    """read_ranges for one range"""
    return read_ranges(blob, [(off, length)], nblocks, block_lens, raw_lens, crcs)[0]


class Decoder:
    """A block container (nblocks streams back to back) decoded in steps on the device: every step is one launch that takes the blocks it
    concerns to a frame boundary, where they stay at rest in a record the library keeps until a later step picks them up.  The container is
    uploaded once and decoded into a buffer of the library's; read() fetches from it.  One Decoder is open at a time (a new one closes the
    one before it); a context manager: leaving it abandons what is not finished.  Without raw_lens the blocks are sized first (a pass of its own)."""

    def __init__(self, blob, nblocks: int = 1, block_lens=None, raw_lens=None):
        lib = load_library()
        src = _bytes_in(blob)
        _one_per_block(nblocks, block_lens=block_lens, raw_lens=raw_lens)
        blen, raw = _arr(C.c_uint64, block_lens), _arr(C.c_uint64, raw_lens)
        if raw is None:          # (the lengths are wanted here too: read() addresses the decoded bytes)
            raw, total = (C.c_uint64 * nblocks)(), C.c_uint64(0)
            _chk(lib.nlzm_hip_decompress_blocks(src.ctypes.data, src.size, nblocks, blen, None, None, 0, raw, C.byref(total)))
        self.nblocks = nblocks
        self.raw_lens = [int(x) for x in raw]
        self.starts = [sum(self.raw_lens[:i]) for i in range(nblocks)]
        self.done = [0] * nblocks
        self.finished = False
        self.device_ms = 0.0
        _chk(lib.nlzm_hip_decode_begin(src.ctypes.data, src.size, nblocks, blen, raw, 0))
        self._open = True

    def step(self, max_frames: int = 0, targets=None):
        """One launch: every block that is neither finished nor at its target advances by at most max_frames frames (0: no limit) and stops at
        the first frame boundary with targets[i] bytes decoded (None, or TO_THE_END: at its end).  (done, finished)."""
        if not self._open:
            raise NlzmError("the decoder is closed")
        if targets is not None and len(targets) != self.nblocks:
            raise ValueError("targets: one entry per block")
        tg = None if targets is None else _arr(C.c_uint64, [min(int(t), TO_THE_END) for t in targets])
        done, fin, ms = (C.c_uint64 * self.nblocks)(), C.c_int(0), C.c_double(0)
        rc = load_library().nlzm_hip_decode_step(max_frames, tg, done, C.byref(fin), C.byref(ms))
        if rc:
            self._open = False       # (a failing step has closed the set)
            _chk(rc)
        self.done, self.finished, self.device_ms = [int(x) for x in done], bool(fin.value), self.device_ms + ms.value
        return list(self.done), self.finished

    def read(self, off: int, length: int) -> bytes:
        """`length` decoded bytes from offset `off` of the container's content: exactly the blocks the range intersects advance, each up to the
        range's end in it (one step), and the bytes are fetched.  A later read further on in a block goes on where this one stopped."""
        total = sum(self.raw_lens)
        if off < 0 or length < 0 or off > total or length > total - off:
            raise ValueError("the range runs over the container's decoded bytes")
        if not length:
            return b""
        targets = list(self.done)
        for i, (lo, n) in enumerate(zip(self.starts, self.raw_lens)):
            if lo < off + length and off < lo + n:
                targets[i] = max(targets[i], min(off + length, lo + n) - lo)
        if any(t > d for t, d in zip(targets, self.done)):
            self.step(0, targets)
        dst = np.empty(length, dtype=np.uint8)
        _chk(load_library().nlzm_hip_decode_fetch(off, length, dst.ctypes.data))
        return dst.tobytes()

    def close(self) -> None:
        if self._open:
            load_library().nlzm_hip_decode_abandon()
            self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def stats() -> dict:
    s = Stats()
    _chk(load_library().nlzm_hip_get_stats(C.byref(s)))
    return s.as_dict()


def counter(key: str) -> int:
    """A diagnostic counter of the pipeline stages for the last stream (nlzm_hip_get_counter)."""
    v = C.c_uint64(0)
    _chk(load_library().nlzm_hip_get_counter(key.encode(), C.byref(v)))
    return int(v.value)


def timing() -> dict:
    t = Timing()
    _chk(load_library().nlzm_hip_get_timing(C.byref(t)))
    return t.as_dict()


def rans_frames(frames: list[tuple[np.ndarray, np.ndarray, int]]) -> list[bytes]:
    """CodeFrame::Flush replacement: frames = [(syms u32, bits u8 incl. pad, num_ops)]."""
    lib = load_library()
    nf = len(frames)
    sym_off = np.zeros(nf + 1, dtype=np.uint64)
    bit_off = np.zeros(nf + 1, dtype=np.uint64)
    for i, (s, b, _) in enumerate(frames):
        sym_off[i + 1] = sym_off[i] + len(s)
        bit_off[i + 1] = bit_off[i] + len(b)
    syms = np.concatenate([np.asarray(s, dtype=np.uint32) for s, _, _ in frames] + [np.zeros(1, np.uint32)])
    bits = np.concatenate([np.asarray(b, dtype=np.uint8) for _, b, _ in frames] + [np.zeros(1, np.uint8)])
    ops = np.array([o for _, _, o in frames], dtype=np.uint32)
    stride = int(max(12 + len(b) + 16 + 2 * len(s) for s, b, _ in frames)) + 16
    out = np.zeros(nf * stride, dtype=np.uint8)
    out_len = np.zeros(nf, dtype=np.uint32)
    _chk(lib.nlzm_hip_rans_frames(syms.ctypes.data, sym_off.ctypes.data, bits.ctypes.data, bit_off.ctypes.data,
                                  ops.ctypes.data, nf, out.ctypes.data, stride, out_len.ctypes.data))
    return [out[i * stride: i * stride + int(out_len[i])].tobytes() for i in range(nf)]


def find_matches(data, hist_bits: int, pos_lo: int, pos_hi: int, cap_words: int = 1 << 24) -> np.ndarray:
    lib = load_library()
    src = _bytes_in(data)
    out = np.empty(cap_words, dtype=np.uint32)
    used = C.c_uint64(0)
    _chk(lib.nlzm_hip_find_matches(src.ctypes.data, src.size, hist_bits, pos_lo, pos_hi, out.ctypes.data, cap_words,
                                   C.byref(used)))
    return out[: used.value].copy()


def parse_emit(data, hist_bits: int, frame_idx: int):
    lib = load_library()
    src = _bytes_in(data)
    syms = np.empty(1 << 19, dtype=np.uint32)
    bits = np.empty(1 << 18, dtype=np.uint8)
    sizes = np.zeros(3, dtype=np.uint32)
    _chk(lib.nlzm_hip_parse_emit(src.ctypes.data, src.size, hist_bits, frame_idx, syms.ctypes.data, syms.size,
                                 bits.ctypes.data, bits.size, sizes.ctypes.data))
    return syms[: sizes[0]].copy(), bits[: sizes[1]].copy(), int(sizes[2])
