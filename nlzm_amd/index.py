"""The sidecar index of a block container (`nlzm c -blocks:k` writes <output>.idx), read in pure Python: no library, no ctypes."""
from __future__ import annotations


def read_index_typed(path):
    """The sidecar index of a block container in every version: (block_lens, raw_lens, crcs or None, elems).  `nlzm c -blocks:k` writes NLZMIDX 1
    (`off len raw` per block), with -crc NLZMIDX 2 (a CRC32 behind them, and the whole file's behind the header's fields), with -elem:E NLZMIDX 3
    (the block's element size behind that; the CRC32s are the RAW bytes').  Versions 1 and 2 have every element size 1.  The structural checks are
    the command line's: offsets back to back, no sum that wraps 64 bits, block lengths summing to the header's n_out and raw lengths to its n_in; an
    element size outside 1, 2, 4, 8 is refused.  ValueError when the file is not such an index."""
    words = open(path, "r").read().split()
    M = 1 << 64

    def num(w, base=10):
        try:
            v = int(w, base)
        except ValueError:
            raise ValueError(f"{path}: {w!r} is not a number") from None
        if not 0 <= v < M:
            raise ValueError(f"{path}: {w} does not fit 64 bits")
        return v

    if len(words) < 2 or words[0] != "NLZMIDX" or words[1] not in ("1", "2", "3"):
        raise ValueError(f"{path}: not an NLZMIDX 1 or 2 file")
    ver = int(words[1])
    head, per = 5 + (ver >= 2), 2 + ver                  # (the header's fields, an entry's)
    if len(words) < (6 if ver == 3 else 5):
        raise ValueError(f"{path}: not an NLZMIDX 3 file" if ver == 3 else f"{path}: not an NLZMIDX 1 or 2 file")
    k, n_in, n_out = num(words[2]), num(words[3]), num(words[4])
    if not 1 <= k <= 65536 or len(words) != head + per * k:
        raise ValueError(f"{path}: {k} blocks do not fit the file's {len(words)} fields")
    if ver >= 2 and num(words[5], 16) >= 1 << 32:
        raise ValueError(f"{path}: the whole file's CRC32 does not fit 32 bits")
    lens, raws, crcs, elems, expect, raw_sum = [], [], [], [], 0, 0
    for i in range(k):
        f = words[head + per * i: head + per * (i + 1)]
        off, ln, raw = num(f[0]), num(f[1]), num(f[2])
        c, e = (num(f[3], 16), num(f[4])) if ver == 3 else (0, 1)
        if off != expect or ln < 8 or off + ln >= M or ln > n_out - expect or raw > n_in - raw_sum:
            raise ValueError(f"{path}: block {i + 1}'s entry does not fit (offset {off}, length {ln}, raw length {raw})")
        if ver == 2:                                     # (read behind the entry's check, as version 2 always was)
            c = num(f[3], 16)
        if c >= 1 << 32:
            raise ValueError(f"{path}: block {i + 1}'s CRC32 does not fit 32 bits")
        if e not in (1, 2, 4, 8):
            raise ValueError(f"{path}: block {i + 1}'s element size {e} is not 1, 2, 4 or 8")
        lens.append(ln)
        raws.append(raw)
        crcs.append(c)
        elems.append(e)
        expect, raw_sum = expect + ln, raw_sum + raw
    if expect != n_out or raw_sum != n_in:
        raise ValueError(f"{path}: the blocks' lengths sum to {expect} / {raw_sum}, the header says {n_out} / {n_in}")
    return lens, raws, (crcs if ver >= 2 else None), elems


def read_index(path):
    """read_index_typed for the versions without typed blocks (NLZMIDX 1 and 2): (block_lens, raw_lens, crcs or None).  Version 3 is refused."""
    words = open(path, "r").read().split()
    if len(words) < 5 or words[0] != "NLZMIDX" or words[1] not in ("1", "2"):
        raise ValueError(f"{path}: not an NLZMIDX 1 or 2 file")
    return read_index_typed(path)[:3]
