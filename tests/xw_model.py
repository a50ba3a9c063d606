"""The model of nlzm_amd/csrc/xw.h: every primitive as plain Python over a list of 64 lane values, from the definition its comment gives
("value of lane - d, own value for the first d lanes", "inclusive prefix", "lane 0: fill"), the input table of the probe role
(tests/xw_probe/xw_probe.h) and the output table that role must produce.  tests/test_xw_sim.py holds the simulation build to it,
tests/test_gpu_xw.py the gfx950 build.  Nothing here is taken from either build's code.

A primitive's model returns (values, defined): `defined[l]` is False for a lane that has left the role and for a live lane whose result
depends on such a lane's value -- xw.h leaves those undefined in both builds, and they are recorded, never asserted."""
import numpy as np

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
LANES = 64
EDGE_LANES = [0, 15, 16, 31, 32, 47, 48, 63]           # both sides of every DPP row boundary
ALL_LIVE = [True] * LANES

# ---- the layout (xw_probe.h) ------------------------------------------------------------------------------------------------------------
MAGIC, THREADS, HEAD, REC, SENTINEL = 0x78775031, 256, 16, 4 + 3 * 64, 0xDEADBEEF
OPS = ["ballot", "any", "readlane", "readlane64", "readfirst", "readfirst64", "shfl", "shfl64", "shfl_up", "shfl_up64", "scan_max", "scan_add",
       "scan_min_i32", "lane_below"]
OP = {n: i + 1 for i, n in enumerate(OPS)}
L_INC, L_INC_FINAL, L_ADD, L_OR, L_MAX, L_ADD64, L_MIN64, L_RT_WAVE, L_RT_BLOCK, L_WORDS = 0, 256, 260, 264, 268, 272, 276, 284, 540, 796
G_WORDS = 3088
EXIT_PATTERNS = [("lanes 40..63 left", [l < 40 for l in range(LANES)]), ("every third lane left", [l % 3 != 0 for l in range(LANES)])]


# ---- the primitives --------------------------------------------------------------------------------------------------------------------
def ballot(pred, live=ALL_LIVE):
    m = sum(1 << l for l in range(LANES) if live[l] and pred[l])      # an exited lane's bit is 0
    return [m] * LANES, list(live)


def any_(pred, live=ALL_LIVE):
    return [int(any(pred[l] for l in range(LANES) if live[l]))] * LANES, list(live)


def readlane(v, lane, live=ALL_LIVE):
    return [v[lane]] * LANES, [live[l] and live[lane] for l in range(LANES)]


def readfirst(v, live=ALL_LIVE):
    first = next(l for l in range(LANES) if live[l])                  # the first lane that is still in the role
    return [v[first]] * LANES, list(live)


def shfl(v, src, live=ALL_LIVE):
    return [v[src[l] & 63] for l in range(LANES)], [live[l] and live[src[l] & 63] for l in range(LANES)]


def shfl_up(v, d, live=ALL_LIVE):
    """value of lane - d, own value for the first d lanes"""
    return shfl(v, [l - d if l >= d else l for l in range(LANES)], live)


def _scan(v, f, live):
    out, acc = [], None
    for l in range(LANES):
        acc = v[l] if l == 0 else f(acc, v[l])
        out.append(acc)
    return out, [all(live[:l + 1]) for l in range(LANES)]             # an inclusive prefix depends on every lane up to its own


def scan_max(v, live=ALL_LIVE):
    return _scan(v, max, live)                                        # unsigned


def scan_add(v, live=ALL_LIVE):
    return _scan(v, lambda a, b: (a + b) & M32, live)                 # wraps at 2^32


def _i32(x):
    return x - (1 << 32) if x & 0x80000000 else x


def scan_min_i32(v, live=ALL_LIVE):
    out, ok = _scan([_i32(x) for x in v], min, live)                  # signed
    return [x & M32 for x in out], ok


def lane_below(v, fill, live=ALL_LIVE):
    """value of the lane below (lane 0: fill)"""
    return [fill if l == 0 else v[l - 1] for l in range(LANES)], [live[l] and (l == 0 or live[l - 1]) for l in range(LANES)]


def apply(case, live=ALL_LIVE):
    """a case's 64 results (as 64-bit values) and which of them the contract defines"""
    op, lo, hi = case["op"], case["lo"], case["hi"]
    v64 = [(h << 32) | l for l, h in zip(lo, hi)]
    if op == "ballot":
        return ballot([x != 0 for x in lo], live)
    if op == "any":
        return any_([x != 0 for x in lo], live)
    if op == "readlane":
        return readlane(lo, case["a"], live)
    if op == "readlane64":
        return readlane(v64, case["a"], live)
    if op == "readfirst":
        return readfirst(lo, live)
    if op == "readfirst64":
        return readfirst(v64, live)
    if op == "shfl":
        return shfl(lo, case["src"], live)
    if op == "shfl64":
        return shfl(v64, case["src"], live)
    if op == "shfl_up":
        return shfl_up(lo, case["a"], live)
    if op == "shfl_up64":
        return shfl_up(v64, case["a"], live)
    if op == "scan_max":
        return scan_max(lo, live)
    if op == "scan_add":
        return scan_add(lo, live)
    if op == "scan_min_i32":
        return scan_min_i32(lo, live)
    if op == "lane_below":
        return lane_below(lo, case["fill"], live)
    raise ValueError(op)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def vectors(rng):
    """(name, 64 words): the inputs every primitive that takes a per-lane value gets"""
    v = [("zero", [0] * LANES), ("ones", [M32] * LANES), ("ascending", list(range(LANES))), ("descending", [63 - l for l in range(LANES)])]
    for s in EDGE_LANES:
        v.append((f"spike{s}", [0xC0000000 + s if l == s else 1 for l in range(LANES)]))
    v.append(("random", [int(x) for x in rng.integers(0, 1 << 32, LANES, dtype=np.uint64)]))
    v.append(("around_2^31", [(0x80000000 + l - 32) & M32 for l in range(LANES)]))           # below 2^31 up to lane 31, at and above it from 32
    v.append(("around_2^31_down", [(0x80000000 + 31 - l) & M32 for l in range(LANES)]))
    return v


def _case(op, name, lo, hi=None, a=0, fill=0, src=None):
    return {"op": op, "name": name, "lo": [int(x) & M32 for x in lo], "hi": [(~int(x)) & M32 for x in lo] if hi is None else [int(x) & M32 for x in hi],
            "a": a, "fill": fill, "src": list(range(LANES)) if src is None else [int(s) for s in src]}


def make_cases(seed=20240607):
    rng = np.random.default_rng(seed)
    vecs = vectors(rng)
    rnd = dict(vecs)["random"]
    big = dict(vecs)["around_2^31"]
    cases = []
    preds = [("none", [0] * LANES), ("all", [1] * LANES)] + [(f"only{s}", [int(l == s) for l in range(LANES)]) for s in EDGE_LANES]
    preds.append(("random", [int(x) for x in rng.integers(0, 2, LANES)]))
    for n, p in preds:
        cases.append(_case("ballot", n, p))
        cases.append(_case("any", n, p))
    for l in EDGE_LANES:
        for n, v in (("ascending", list(range(LANES))), ("random", rnd), ("around_2^31", big)):
            cases.append(_case("readlane", f"{n}_l{l}", v, a=l))
            cases.append(_case("readlane64", f"{n}_l{l}", v, a=l))          # (hi = ~lo: the halves differ)
    for n, v in vecs:
        cases.append(_case("readfirst", n, v))
        cases.append(_case("readfirst64", n, v))
    maps = [("identity", list(range(LANES))), ("reversal", [63 - l for l in range(LANES)])]
    maps += [(f"rotate{r}", [(l + r) & 63 for l in range(LANES)]) for r in (1, 16, 32)]
    maps += [("all_to_0", [0] * LANES), ("all_to_63", [63] * LANES), ("permutation", [int(x) for x in rng.permutation(LANES)]),
             ("non_injective", [int(x) for x in rng.integers(0, LANES, LANES)]), ("lane_plus_64", [l + 64 for l in range(LANES)]),
             ("rotate1_plus_192", [((l + 1) & 63) + 192 for l in range(LANES)])]
    for n, m in maps:
        for vn, v in (("ascending", list(range(LANES))), ("random", rnd), ("around_2^31", big)):
            cases.append(_case("shfl", f"{n}_{vn}", v, src=m))
            cases.append(_case("shfl64", f"{n}_{vn}", v, src=m))
    for d in (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64):
        for vn, v in (("ascending", list(range(LANES))), ("random", rnd), ("around_2^31", big)):
            cases.append(_case("shfl_up", f"d{d}_{vn}", v, a=d))
            cases.append(_case("shfl_up64", f"d{d}_{vn}", v, a=d))
    for n, v in vecs:
        cases.append(_case("scan_max", n, v))
        cases.append(_case("scan_add", n, v))
        cases.append(_case("scan_min_i32", n, v))
    # sums that wrap 2^32: at once, in the middle, in every row
    cases.append(_case("scan_add", "wrap_all_0x80000000", [0x80000000] * LANES))
    cases.append(_case("scan_add", "wrap_big_random", [int(x) | 0xF0000000 for x in rng.integers(0, 1 << 32, LANES, dtype=np.uint64)]))
    cases.append(_case("scan_add", "wrap_at_lane_16", [0xFFFFFFF0 if l == 0 else 1 for l in range(LANES)]))
    cases.append(_case("scan_add", "wrap_at_lane_48", [0xFFFFFFD0 if l == 0 else 1 for l in range(LANES)]))
    INT_MIN, INT_MAX = 0x80000000, 0x7FFFFFFF
    cases.append(_case("scan_min_i32", "all_INT_MAX", [INT_MAX] * LANES))
    cases.append(_case("scan_min_i32", "all_INT_MIN", [INT_MIN] * LANES))
    cases.append(_case("scan_min_i32", "all_minus_1", [M32] * LANES))
    for s in EDGE_LANES:
        cases.append(_case("scan_min_i32", f"INT_MIN_at_{s}", [INT_MIN if l == s else INT_MAX for l in range(LANES)]))
        cases.append(_case("scan_min_i32", f"minus_1_at_{s}", [M32 if l == s else l for l in range(LANES)]))
    cases.append(_case("scan_min_i32", "random_signed", rnd))
    # the shape the parser uses: (int32) mc - (int32) S, mc at the parser's kInf, S ascending; then with finite costs among them
    k_inf = 0x3FFFFFFF
    cases.append(_case("scan_min_i32", "kInf_minus_S", [(k_inf - 1000 * l) & M32 for l in range(LANES)]))
    cases.append(_case("scan_min_i32", "cost_minus_S", [((k_inf if l % 5 else 40000 + int(rng.integers(0, 5000))) - 3000 * l) & M32 for l in range(LANES)]))
    for n, v in vecs:
        cases.append(_case("lane_below", n, v, fill=0x0F1E2D3C))                              # a fill that occurs in no lane
    return cases


def make_exit_cases(seed=20240608):
    """what the waves with exited lanes run; live in BOTH patterns: the lanes below 40 that are no multiple of 3"""
    rng = np.random.default_rng(seed)
    asc = [0x100 + l for l in range(LANES)]
    rnd = [int(x) for x in rng.integers(0, 1 << 32, LANES, dtype=np.uint64)]
    both = [l for l in range(40) if l % 3]
    cases = [_case("ballot", "all", [1] * LANES), _case("ballot", "random", [int(x) for x in rng.integers(0, 2, LANES)]), _case("ballot", "none", [0] * LANES),
             _case("any", "only_lane_0", [int(l == 0) for l in range(LANES)]), _case("any", "only_lane_63", [int(l == 63) for l in range(LANES)]),
             _case("any", "only_lane_1", [int(l == 1) for l in range(LANES)])]
    for l in (1, 16, 0, 39, 47, 63):
        cases.append(_case("readlane", f"ascending_l{l}", asc, a=l))
        cases.append(_case("readlane64", f"random_l{l}", rnd, a=l))
    for v, n in ((asc, "ascending"), (rnd, "random")):
        cases.append(_case("readfirst", n, v))
        cases.append(_case("readfirst64", n, v))
        cases.append(_case("shfl", f"identity_{n}", v))
        cases.append(_case("shfl64", f"live_sources_{n}", v, src=[both[int(x)] for x in rng.integers(0, len(both), LANES)]))
        cases.append(_case("shfl", f"rotate1_{n}", v, src=[(l + 1) & 63 for l in range(LANES)]))
        cases.append(_case("shfl", f"all_to_1_{n}", v, src=[1] * LANES))
        cases.append(_case("shfl", f"all_to_63_{n}", v, src=[63] * LANES))
        for d in (0, 1, 3, 16):
            cases.append(_case("shfl_up", f"d{d}_{n}", v, a=d))
        cases.append(_case("shfl_up64", f"d3_{n}", v, a=3))
        cases.append(_case("scan_max", n, v))
        cases.append(_case("scan_add", n, v))
        cases.append(_case("scan_min_i32", n, v))
        cases.append(_case("lane_below", n, v, fill=0x0F1E2D3C))
    return cases


def thread_inputs(seed=20240609):
    """per thread: x, the lds_min64 operand's halves, y"""
    rng = np.random.default_rng(seed)
    x = [int(v) for v in rng.integers(0, 1 << 32, THREADS, dtype=np.uint64)]
    y = [int(v) for v in rng.integers(0, 1 << 32, THREADS, dtype=np.uint64)]
    r = [int(v) for v in rng.integers(0, 1 << 32, 2 * THREADS, dtype=np.uint64)]
    mlo, mhi = [], []
    for t in range(THREADS):
        k = t & 3
        if k == 0:          # the values differ only in the high half (bit 31 of it set in some: the compare is unsigned)
            mlo.append(0x12345678); mhi.append(r[t] | 0x100)
        elif k == 1:        # ... only in the low half
            mlo.append(r[t] | 0x100); mhi.append(0x80000000)
        elif k == 2:        # the high half decides against the low one
            mlo.append(M32 - t); mhi.append(5 + t)
        else:
            mlo.append(r[t]); mhi.append(r[THREADS + t])
    return x, mlo, mhi, y


class Table:
    """the probe's input, and everything the output must be"""

    def __init__(self, strict):
        self.cases, self.exit_cases = make_cases(), make_exit_cases()
        self.nc, self.ne, self.strict = len(self.cases), len(self.exit_cases), int(strict)
        self.x, self.mlo, self.mhi, self.y = thread_inputs()
        nc, ne = self.nc, self.ne
        self.in_thread = HEAD + (nc + ne) * REC
        self.o_case = 3 * THREADS
        self.o_lds = self.o_case + nc * 128
        self.o_agent = self.o_lds + L_WORDS
        self.o_misc = self.o_agent + 16 * THREADS
        self.o_exit = self.o_misc + 4 * THREADS
        self.out_words = self.o_exit + 2 * ne * 128
        self.out2_words = 32 * THREADS
        self.g_final = {}                                               # the two 16-byte slots of every thread
        for t in range(THREADS):
            a = [self.x[t], self.x[t] ^ 0x11111111, ~self.x[t] & M32, (self.x[t] + 0x01010101) & M32]
            self.g_final[t] = (a, [~a[0] & M32, (a[1] + 0x9E3779B9) & M32, a[2] ^ 0xFFFF0000, (a[3] * 5 + 1) & M32])
        self.exit_model = [[apply(c, live) for c in self.exit_cases] for _, live in EXIT_PATTERNS]
        # strict: a case in which a live lane would read an exited one is not run (bit p of the flags: pattern p)
        self.exit_flags = [sum(1 << p for p, (_, live) in enumerate(EXIT_PATTERNS) if any(live[l] and not self.exit_model[p][i][1][l] for l in range(LANES)))
                           for i in range(ne)]

    def input(self):
        w = np.zeros(self.in_thread + 4 * THREADS, dtype=np.uint32)
        w[:4] = [MAGIC, self.nc, self.ne, self.strict]
        for i, c in enumerate(self.cases + self.exit_cases):
            o = HEAD + i * REC
            w[o:o + 4] = [OP[c["op"]], c["a"], c["fill"], self.exit_flags[i - self.nc] if i >= self.nc else 0]
            w[o + 4:o + 68] = c["lo"]
            w[o + 68:o + 132] = c["hi"]
            w[o + 132:o + 196] = c["src"]
        for t in range(THREADS):
            w[self.in_thread + 4 * t:self.in_thread + 4 * t + 4] = [self.x[t], self.mlo[t], self.mhi[t], self.y[t]]
        return w

    # -- what phase 0 must write: (want, asserted, label) per word; label = (section, case, slot) --
    def expected(self):
        n = self.out_words
        want = np.full(n, SENTINEL, dtype=np.uint32)
        check = np.zeros(n, dtype=bool)
        label = [None] * n

        def put(i, v, lab, asserted=True):
            want[i], check[i], label[i] = v & M32, asserted, lab

        for t in range(THREADS):
            for k, (nm, v) in enumerate((("lane()", t & 63), ("wave()", t >> 6), ("thread()", t))):
                put(3 * t + k, v, (nm, "identity", f"thread {t}"))
        for i, c in enumerate(self.cases):
            vals, _ = apply(c)
            for l in range(LANES):
                put(self.o_case + i * 128 + 2 * l, vals[l], (c["op"], c["name"], f"lane {l} low word"))
                put(self.o_case + i * 128 + 2 * l + 1, vals[l] >> 32, (c["op"], c["name"], f"lane {l} high word"))
        x, y, o = self.x, self.y, self.o_lds
        for t in range(THREADS):
            put(o + L_INC + t, 0, ("lds_inc", "returned", f"thread {t}"), False)              # a property: see check_properties
            put(o + L_RT_WAVE + t, x[(t & ~63) | ((t + 1) & 63)] ^ 0x5A5A5A5A, ("lds_st/lds_ld", "across wave_sync", f"thread {t}"))
            put(o + L_RT_BLOCK + t, x[(t + 64) & 255] ^ 0x5A5A5A5A, ("lds_st/lds_ld", "across block_sync", f"thread {t}"))
        put(o + L_INC_FINAL, THREADS, ("lds_inc", "final", "word"))
        for k in range(4):
            mine = [t for t in range(THREADS) if t & 3 == k]
            put(o + L_ADD + k, sum(x[t] for t in mine), ("lds_add", "final", f"word {k}"))
            orv = 0
            for t in mine:
                orv |= y[t]
            put(o + L_OR + k, orv, ("lds_or", "final", f"word {k}"))
            put(o + L_MAX + k, max(x[t] for t in mine), ("lds_max", "final", f"word {k}"))
            m = min(min((self.mhi[t] << 32) | self.mlo[t] for t in mine), M64)
            put(o + L_MIN64 + 2 * k, m, ("lds_min64", "final", f"word {k} low half"))
            put(o + L_MIN64 + 2 * k + 1, m >> 32, ("lds_min64", "final", f"word {k} high half"))
        for k in range(2):
            s = (THREADS // 2) * M32
            put(o + L_ADD64 + 2 * k, s, ("lds_add64", "final", f"word {k} low half"))
            put(o + L_ADD64 + 2 * k + 1, s >> 32, ("lds_add64", "final", f"word {k} high half"))
        for t in range(THREADS):
            o = self.o_agent + 16 * t
            a, b = self.g_final[t]
            for k in range(4):
                put(o + k, a[k], ("st_agent128/ld_agent128", "first slot", f"thread {t} word {k}"))
                put(o + 4 + k, b[k], ("st_agent128/ld_agent128", "second slot (variables overwritten behind the first store)", f"thread {t} word {k}"))
            put(o + 8, y[t], ("st_agent/ld_agent", "own word", f"thread {t}"))
            put(o + 9, y[t], ("st_agent64/ld_agent64", "own word", f"thread {t} low half"))
            put(o + 10, ~y[t], ("st_agent64/ld_agent64", "own word", f"thread {t} high half"))
            put(o + 11, 0, ("cas_agent", "uncontended hit, returned", f"thread {t}"))
            put(o + 12, 1000 + t, ("cas_agent", "uncontended miss, returned", f"thread {t}"))
            put(o + 13, 0, ("cas_agent", "contended, returned", f"thread {t}"), False)         # a property
            m = self.o_misc + 4 * t
            put(m, x[t], ("opaque", "value", f"thread {t}"))
            put(m + 1, 1, ("tick", "second not below the first", f"thread {t}"))
            put(m + 2, 1, ("clock100", "second not below the first", f"thread {t}"))
            put(m + 3, 0xC0FFEE, ("role", "reached the end of the uniform part", f"thread {t}"))
        for p, (pname, live) in enumerate(EXIT_PATTERNS):
            for i, c in enumerate(self.exit_cases):
                vals, ok = self.exit_model[p][i]
                skipped = self.strict and (self.exit_flags[i] >> p) & 1
                for l in range(LANES):
                    for h in range(2):
                        j = self.o_exit + (p * self.ne + i) * 128 + 2 * l + h
                        lab = (c["op"], f"{c['name']} with {pname}", f"lane {l} {'high' if h else 'low'} word")
                        if not live[l] or skipped:
                            put(j, SENTINEL, lab)                       # an exited lane writes nothing; nor does a case that is left out
                        else:
                            put(j, vals[l] >> (32 * h), lab, ok[l])     # undefined: recorded, not asserted
        return want, check, label

    def expected2(self):
        """phase 1: what phase 0 left in the shared words, by plain loads and by the agent-scope ones"""
        n = self.out2_words
        want = np.zeros(n, dtype=np.uint32)
        check = np.ones(n, dtype=bool)
        label = [None] * n
        x, y = self.x, self.y
        for t in range(THREADS):
            a, b = self.g_final[t]
            row = a + b + a + b + [y[t], y[t], y[t], ~y[t] & M32, y[t], ~y[t] & M32, 1000 + t]
            k = t & 3
            orv = 0
            for u in range(k, THREADS, 4):
                orv |= y[u]
            s = (THREADS // 2) * M32
            row += [orv, s & M32, s >> 32, 0, 0, 0, 0, 0, 0]
            names = ([f"plain load of the first slot, word {k}" for k in range(4)] + [f"plain load of the second slot, word {k}" for k in range(4)]
                     + [f"ld_agent128 of the first slot, word {k}" for k in range(4)] + [f"ld_agent128 of the second slot, word {k}" for k in range(4)]
                     + ["ld_agent of st_agent's word", "plain load of st_agent's word", "ld_agent64 low", "ld_agent64 high", "plain 64-bit load low",
                        "plain 64-bit load high", "cas_agent's word (the hit's value)", "atomic_or_agent's word", "atomic_add64_agent's word low",
                        "atomic_add64_agent's word high", "the contended cas_agent's word"] + ["unused"] * 5)
            for k in range(32):
                want[32 * t + k], label[32 * t + k] = row[k] & M32, ("second launch", names[k], f"thread {t}")
            check[32 * t + 26] = False                                  # a property
        return want, check, label


def compare(got, want, check, label, limit=20):
    """the asserted words of a table against the model's, word for word: one message per mismatch, naming primitive, case, lane, got, want"""
    got = np.asarray(got, dtype=np.uint32)
    if got.shape != want.shape:
        return [f"the table has {got.size} words, the model's {want.size}"]
    bad = np.flatnonzero((got != want) & check)
    return [f"{label[i][0]}: case {label[i][1]}, {label[i][2]}: got 0x{int(got[i]):08X}, want 0x{int(want[i]):08X}" for i in bad[:limit]] + \
           ([f"... and {bad.size - limit} more"] if bad.size > limit else [])


def check_properties(T, out0, out1):
    """what the hardware orders: lds_inc hands out 0 .. 255 once each; of the contended cas_agent exactly one thread is returned 0 and the word
    holds that thread's value, which is what every other thread was returned"""
    msgs = []
    inc = sorted(int(v) for v in out0[T.o_lds + L_INC:T.o_lds + L_INC + THREADS])
    if inc != list(range(THREADS)):
        msgs.append(f"lds_inc: the returned values are no permutation of 0 .. 255: {inc[:8]} ...")
    ret = [int(out0[T.o_agent + 16 * t + 13]) for t in range(THREADS)]
    winners = [t for t in range(THREADS) if ret[t] == 0]
    if len(winners) != 1:
        msgs.append(f"cas_agent, contended: {len(winners)} threads were returned 0")
    else:
        w = winners[0] + 1
        others = {ret[t] for t in range(THREADS) if t != winners[0]}
        if others != {w}:
            msgs.append(f"cas_agent, contended: thread {winners[0]} won, the others were returned {sorted(others)[:5]}, not {w}")
        words = {int(out1[32 * t + 26]) for t in range(THREADS)}
        if words != {w}:
            msgs.append(f"cas_agent, contended: thread {winners[0]} won, the second launch reads {sorted(words)[:5]}, not {w}")
    return msgs


def undefined_slots(T, out0):
    """what a build returned where the contract defines nothing: text for the evidence file, one line per exit case and pattern"""
    lines = []
    for p, (pname, live) in enumerate(EXIT_PATTERNS):
        for i, c in enumerate(T.exit_cases):
            vals, ok = T.exit_model[p][i]
            slots = [l for l in range(LANES) if live[l] and not ok[l]]
            if not slots:
                continue
            base = T.o_exit + (p * T.ne + i) * 128
            if int(out0[base + 2 * slots[0]]) == SENTINEL and int(out0[base + 2 * slots[0] + 1]) == SENTINEL:
                lines.append(f"{c['op']:13s} {c['name']:24s} {pname}: not run")
                continue
            kinds = {}
            for l in slots:
                got = int(out0[base + 2 * l]) | (int(out0[base + 2 * l + 1]) << 32)
                own = c["lo"][l] | ((c["hi"][l] << 32) if c["op"].endswith("64") else 0)
                kind = ("what the exited lane would have supplied" if got == vals[l] else "the lane's own input" if got == own else
                        "the fill" if c["op"] == "lane_below" and got == c["fill"] else "0" if got == 0 else f"0x{got:X}")
                kinds.setdefault(kind, []).append(l)
            lines.append(f"{c['op']:13s} {c['name']:24s} {pname}: " + "; ".join(f"{k} in lanes {v[:6]}{' ...' if len(v) > 6 else ''} ({len(v)})" for k, v in kinds.items()))
    return lines
