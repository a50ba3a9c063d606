"""The C ABI of libnlzm_hip.so as ctypes sees it: one row per function of include/nlzm_hip.h, name -> (restype, argtypes).

A host-buffer entry and its `_dev` twin take the same list and are declared together.  tests/test_abi.py parses the header's prototypes and
holds every row to them (widths, signedness, pointer positions, pointee types), so a new entry point is one prototype there and one row here.
ELEM_TABLE is the same for include/nlzm_hip_elem.h (the element sizes of typed ranges chosen on the device), held by tests/test_elem_abi.py.
bind() gives a loaded library the rows of the symbols it exports: a build of an earlier commit, loaded through NLZM_LIB for an A/B run, lacks
the newer ones and loads all the same.
"""
from __future__ import annotations

import ctypes as C


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "in_bytes", "out_bytes", "bt_calls", "bt_tests", "cmp_bytes", "ht_rows", "rk_probes", "rk_inserts",
        "positions", "nice_positions", "segments", "n_literal", "n_dict", "n_rep", "rans_syms", "bit_ops",
        "frames", "shifts", "uncertain_positions")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double), ("prep_ms", C.c_double),
                ("match_parse_ms", C.c_double), ("rans_ms", C.c_double), ("match_parse_launches", C.c_uint32),
                ("rans_launches", C.c_uint32), ("prep_launches", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


i32, i64, u32, u64, vp, text = C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_char_p
i32p, f64p, u8p, u32p, u64p = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)

TABLE: dict[str, tuple] = {}


def _row(names: str, restype, *argtypes) -> None:
    for name in names.split():
        TABLE["nlzm_hip_" + name] = (restype, list(argtypes))


# buffers are c_void_p wherever the callers pass an address (numpy's .ctypes.data, torch's data_ptr()); host arrays made with ctypes are typed
_row("init", i32, i32)
_row("shutdown", None)
_row("last_error", text)
_row("compress_bound", u64, u64)
_row("geometry", None, u64, u32, u32p, u32p, u32p, u32p)
_row("compress compress_dev", i32, vp, u64, u32, vp, u64, u64p)
_row("stream_begin", i32, vp, u64, u32, vp, u64)
_row("stream_step", i32, u32, u64p, u64p, i32p)
_row("stream_finish", i32, u64p)
_row("get_stats", i32, C.POINTER(Stats))
_row("get_timing", i32, C.POINTER(Timing))
_row("get_counter", i32, text, u64p)
_row("rans_frames", i32, vp, vp, vp, vp, vp, u32, vp, u64, vp)
_row("find_matches", i32, vp, u64, u32, u64, u64, vp, u64, u64p)
_row("parse_emit", i32, vp, u64, u32, u32, vp, u32, vp, u32, vp)
_row("set_option", i32, text, i64)
_row("blocks_begin", i32, vp, u64, u32, u32)
_row("blocks_step", i32, u32, u64p, i32p, f64p)
_row("blocks_finish", i32, vp, u64, u64p, u64p)
_row("blocks_abandon", None)
_row("compress_blocks compress_blocks_dev", i32, vp, u64, u32, u32, vp, u64, u64p, u64p)
_row("compress_blocks_bound", u64, u64, u32)
_row("compress_blocks_multi", i32, i32p, u32, u32, vp, u64, u32, vp, u64, u64p, u64p)
_row("block_placement", None, u32, u32, u32, u32p, u32p)
_row("feed_begin", i32, u64, u32)
_row("feed", i32, vp, u64)
_row("feed_output", i32, vp, u64, u64p)
_row("feed_finish", i32)
_row("feed_end", None)
_row("feed_input_crc32", i32, u32p)
_row("compress_ranges compress_ranges_dev", i32, vp, u64, u32, u64p, u64p, u32, vp, u64, u64p, u64p)
_row("compress_ranges_bound", u64, u32, u64p)
_row("cut_points cut_points_dev", i32, vp, u64, u32, u64, u64, u64p, u32, u32p)
_row("equal_ranges equal_ranges_dev", i32, vp, u64, u32, u64p, u64p, u32p, u64p)
_row("planes planes_dev", i32, vp, u64, vp, u64, u32, u64p, u64p, u64p, u8p, i32)
_row("compress_ranges_typed compress_ranges_typed_dev", i32, vp, u64, u32, u64p, u64p, u8p, u32, vp, u64, u64p, u64p)
_row("decompress_blocks_typed decompress_blocks_typed_dev", i32, vp, u64, u32, u64p, u64p, u8p, vp, u64, u64p, u64p)
_row("decompress decompress_dev", i32, vp, u64, vp, u64, u64p)
_row("decompress_blocks decompress_blocks_dev", i32, vp, u64, u32, u64p, u64p, vp, u64, u64p, u64p)
_row("verify verify_dev", i32, vp, u64, u32, u64p, vp, u64, u64p, u64p)
_row("decode_begin_dev", i32, vp, u64, u32, u64p, u64p, vp, u64, u32)
_row("decode_begin", i32, vp, u64, u32, u64p, u64p, u32)
_row("decode_step", i32, u32, u64p, u64p, i32p, f64p)
_row("decode_extend_dev", i32, u64)
_row("decode_fetch", i32, u64, u64, vp)
_row("decode_finish", i32, u64p, u64p)
_row("decode_abandon", None)
_row("crc32 crc32_dev", i32, vp, u64, u32, u32p)
_row("crc32_ranges crc32_ranges_dev", i32, vp, u64, u32, u64p, u64p, u32p)
_row("crc32_combine", u32, u32, u32, u64)
_row("check check_dev", i32, vp, u64, u32, u64p, u64p, u32p, u32p, u32p)
_row("read_ranges read_ranges_dev", i32, vp, u64, u32, u64p, u64p, u32p, u32, u64p, u64p, vp, u64, u64p, u32p)

ABI_SYMBOLS = list(TABLE)      # every symbol include/nlzm_hip.h declares

# include/nlzm_hip_elem.h, a header of its own (tests/test_elem_abi.py holds these rows to it as tests/test_abi.py holds the ones above to theirs)
ELEM_TABLE: dict[str, tuple] = {}


def _elem_row(names: str, restype, *argtypes) -> None:
    for name in names.split():
        ELEM_TABLE["nlzm_hip_" + name] = (restype, list(argtypes))


_elem_row("plane_costs plane_costs_dev", i32, vp, u64, u32, u64p, u64p, u64p, u64p)
_elem_row("choose_elem", u32, u64p, u64)
_elem_row("choose_elems choose_elems_dev", i32, vp, u64, u32, u64p, u64p, u8p)
_elem_row("compress_ranges_auto compress_ranges_auto_dev", i32, vp, u64, u32, u64p, u64p, u8p, u32, vp, u64, u64p, u64p)

ELEM_SYMBOLS = list(ELEM_TABLE)


def bind(lib: C.CDLL) -> C.CDLL:
    """Give every symbol of both tables that `lib` exports its restype and argtypes; a symbol it lacks is skipped (and fails where it is called)."""
    for name, (restype, argtypes) in {**TABLE, **ELEM_TABLE}.items():
        try:
            f = getattr(lib, name)
        except AttributeError:
            continue
        f.restype, f.argtypes = restype, argtypes
    return lib
