"""What the tests that drive the command line share: running it, and writing a sidecar index (NLZMIDX 1, 2 or 3) that is right or wrong in a
chosen way.  The layout here is the tests' own restatement of the format; the product's is nlzm_amd/csrc/nlzm_index.h."""
import subprocess

import nlzm_amd


def cli(*args):
    return subprocess.run([nlzm_amd.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True)


def index_text(streams, raws, crcs=None, whole=0, version=2, n_in=None, n_out=None, offs=None, elems=None):
    """`streams`: every block's stream, or its length.  Version 1 holds `off len raw` a block, version 2 a CRC32 behind them and behind the header's
    fields, version 3 the block's element size behind that.  n_in, n_out and offs replace what the blocks add up to; offsets run on modulo 2^64."""
    lens = [len(s) if isinstance(s, bytes) else s for s in streams]
    head = f"NLZMIDX {version} {len(lens)} {sum(raws) if n_in is None else n_in} {sum(lens) if n_out is None else n_out}"
    lines = [head + (f" {whole:08X}" if version >= 2 else "")]
    off = 0
    for i, (ln, raw) in enumerate(zip(lens, raws)):
        entry = f"{off if offs is None else offs[i]} {ln} {raw}"
        if version >= 2:
            entry += f" {crcs[i]:08X}"
        if version >= 3:
            entry += f" {elems[i]}"
        lines.append(entry)
        off = (off + ln) % (1 << 64)
    return "\n".join(lines) + "\n"


def write_index(path, streams, raws, crcs=None, whole=0, **kw):
    path.write_text(index_text(streams, raws, crcs, whole, **kw))
