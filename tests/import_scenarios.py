"""Helper for tests/test_import_paths.py (not a test module).

* The import scanner's constants, read from k2h_import_dev.hip, so that every scenario below is
  built from them and moves with them.
* ref_scan(): the two std::getline loops of k2himport (ConvertfromTsv / ConvertfromMdbm) restated
  with bytes.find, each field cut at its first NUL -- the reference every scanner here (host and
  device) is compared with.  It shares no code with k2h_import.cc.
* span_model(): what the device passes derive from a file -- per 128-byte span its events, whether
  it is packed or over, its cuts and the speculative slots pass A names (in-span, open, head); per
  8 KiB unit the ranks of those slots, the record ends, nrec and staged / direct; per block the
  speculative key count; per key whether pass B takes pass A's state (hit) or hashes it from the
  file (miss), and why.  summary() condenses a model into the quantities the scenarios claim.
* One scenario builder per row of the matrix, each scenario a
  (data, fmt, claims) triple; claims are checked against summary() on the CPU.
* place() / run_scan() / check(): a file on the device between canary bytes that are themselves
  events, one arm of the C ABI into sentinel-filled outputs, and the contract of every arm.
"""
import ctypes
import re
from collections import Counter, namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
_SRC = (ROOT / "k2hash_amd" / "csrc" / "k2h_import_dev.hip").read_text()


def _const(name, env=None):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", _SRC)
    assert m, name
    expr = re.sub(r"(?<=\d)(ull|u|ul)\b", "", m.group(1).strip(), flags=re.I)
    assert re.fullmatch(r"[\w\s*<>+()/]+", expr), (name, expr)
    return int(eval(expr, {"__builtins__": {}}, dict(env or {})))  # noqa: S307  (numbers, names, operators)


T = kTBytes = _const("kTBytes")                      # bytes per span (128)
kTThreads = _const("kTThreads")                      # spans per block (128)
B = kTChunk = _const("kTChunk", dict(kTThreads=kTThreads, kTBytes=kTBytes))   # bytes per block (16 KiB)
U = kUnit = _const("kUnit", dict(kTBytes=kTBytes))   # bytes per pass-B unit (8 KiB)
EC = kEvCap = _const("kEvCap")                       # events a packed span holds (6)
kPre = _const("kPre")                                # bytes before a block the head key may start in (64)
SL = kSpecLenMax = _const("kSpecLenMax")             # longest key a slot holds (254)
kSlots = _const("kSlots")
US = kUnitSlots = _const("kUnitSlots", dict(kSlots=kSlots))   # slot states stored per unit (128)
SR = kStageRecs = _const("kStageRecs")               # records a staged unit holds (96)
kTilePer = _const("kTilePer")
kHdrRecs = _const("kHdrRecs")                        # machine records the mdbm header makes (3)
SPU = U // T                                         # spans per unit (one wave: 64)

EINVAL = -1
PAD = 128
CANARIES = (0x0A, 0x09, 0x00, 0xA5)
SHIFTS = (0, 1, 15)
SENTINEL = 0x5A5AA5A55A5AA5A5
GUARD = 64
ARMS = ("scan", "fused", "fused-h1", "count", "scan+prehash")
HDR74 = b"format=print\ntype=btree\nmdbm_pagesize=4096\nmdbm_pagecount=1\nHEADER=END\n"
END = b"HEADER=END"
NLc, TABc, NULc = 1, 2, 3


# ------------------------------------------------------------------------------ the reference
def _cstr(data, b, e):
    z = data.find(b"\0", b, e)
    return (z if z >= 0 else e) - b


def ref_scan(data, fmt):
    """(error, records): records as (key_off, key_len, val_off, val_len) tuples.

    TSV: while (getline(key, TAB)) { if (eof) break; getline(value); Set(key, value); }
    mdbm: five getline(header); header[4] must be "HEADER=END"; while (getline(key)) {
    getline(value); Set(key, value); } -- a value getline on a stream whose key getline set
    eofbit fails in its sentry and leaves the previous value (reported with its own range; the
    empty string before the first record is reported at the key's offset, length 0).  A value
    getline on a good stream with nothing left extracts nothing: the empty string at offset size.
    """
    data = bytes(data)
    n = len(data)
    recs = []
    p = 0
    if fmt == "tsv":
        while p < n:
            t = data.find(b"\t", p)
            if t < 0:
                break
            kb, p = p, t + 1
            e = data.find(b"\n", p)
            ve = e if e >= 0 else n
            recs.append((kb, _cstr(data, kb, t), p, _cstr(data, p, ve)))
            p = ve + 1
        return False, recs
    assert fmt == "mdbm"
    line4 = None
    for i in range(5):
        if p >= n:
            return True, []          # a header getline failed: header[4] stays empty
        e = data.find(b"\n", p)
        le = e if e >= 0 else n
        if i == 4:
            line4 = data[p:le]
        p = le + 1 if e >= 0 else n
    if line4 != END:
        return True, []
    prev = None
    while p < n:
        e = data.find(b"\n", p)
        if e < 0:                    # the key line ends at EOF: eofbit, the value getline fails
            recs.append((p, _cstr(data, p, n)) + (prev if prev is not None else (p, 0)))
            break
        kb, p = p, e + 1
        e2 = data.find(b"\n", p)
        ve = e2 if e2 >= 0 else n
        prev = (p, _cstr(data, p, ve))
        recs.append((kb, _cstr(data, kb, e)) + prev)
        p = ve + 1 if e2 >= 0 else n
    return False, recs


def recs_array(recs):
    return np.array(recs, np.uint64).reshape(-1, 4)


def oracle_hashes(oracle, data, recs, std_fnv=False):
    """k2h_hash / k2h_second_hash of key + NUL for every record, from the oracle."""
    if not recs:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    keys = b"".join(data[o:o + ln] + b"\0" for o, ln, _, _ in recs)
    off = np.concatenate([[0], np.cumsum([ln + 1 for _, ln, _, _ in recs])]).astype(np.uint64)
    return oracle.hash_csr(np.frombuffer(keys, np.uint8), off, 1 if std_fnv else 0)


# ---------------------------------------------------------------------------------- the model
Slot = namedtuple("Slot", "start len kind rank")   # kind: "in" | "open" | "head"


def span_model(data, fmt="tsv"):
    """What tsv_a_kernel / tsv_b_kernel derive from the file (see the module docstring)."""
    data = bytes(data)
    n = len(data)
    mdbm = fmt == "mdbm"
    a = np.frombuffer(data, np.uint8)
    ty = np.zeros(n, np.uint8)
    ty[a == 10] = NLc
    ty[a == 0] = NULc
    if not mdbm:
        ty[a == 9] = TABc
    pos = np.flatnonzero(ty)
    typ = ty[pos]
    nspan = (n + T - 1) // T
    nunit = (n + U - 1) // U
    nblk = (n + B - 1) // B
    lo = np.searchsorted(pos, np.arange(nspan) * T)
    hi = np.searchsorted(pos, (np.arange(nspan) + 1) * T)
    # false candidates of cand_bits: a 0x0B byte that a borrow from the byte below it, in the same
    # 32-bit word of the file, reaches; and the candidates that are no events (0x01-0x08)
    false_c = np.zeros(n, bool)
    for i in np.flatnonzero(a == 0x0B).tolist():
        if i % 4 and (a[i - 1] < 0x0B or false_c[i - 1]):
            false_c[i] = True
    cand = (a < 0x0B) | false_c
    spans = []
    for s in range(nspan):
        ev = [(int(p) - s * T, int(t)) for p, t in zip(pos[lo[s]:hi[s]], typ[lo[s]:hi[s]])]
        sp = dict(ev=ev, ne=len(ev), over=len(ev) > EC, ends=0, slots=[None, None, None],
                  cands=int(cand[s * T:(s + 1) * T].sum()), false=int(false_c[s * T:(s + 1) * T].sum()))
        sp["cuts"] = [i for i, (_, t) in enumerate(ev) if t >= TABc]
        sp["cut_after_nl"] = [c < 3 and i > 0 and ev[i - 1][1] == NLc for c, i in enumerate(sp["cuts"])][:3]
        spans.append(sp)
    # pass A's speculative slots (TSV only)
    if not mdbm:
        for b in range(nblk):
            has, opn, lpos = False, True, 0          # the newline state, composed in file order
            for s in range(b * kTThreads, min((b + 1) * kTThreads, nspan)):
                sp, ev, base = spans[s], spans[s]["ev"], s * T
                if not sp["over"]:
                    for c, i in enumerate(sp["cuts"][:3]):
                        if i > 0 and ev[i - 1][1] == NLc:
                            st = ev[i - 1][0] + 1
                            sp["slots"][c] = Slot(base + st, ev[i][0] - st, "in", None)
                    if ev and ev[0][1] >= TABc and ((has and opn) or (not has and opn and lpos == 0)):
                        cut0 = base + ev[0][0]
                        if has:
                            start, kind = lpos + 1, "open"
                        elif b == 0:
                            start, kind = 0, "head"
                        else:
                            q = data.rfind(b"\n", b * B - kPre, b * B)
                            start, kind = (q + 1 if q >= 0 else None), "head"
                        if start is not None and cut0 - start <= SL:
                            sp["slots"][0] = Slot(start, cut0 - start, kind, None)
                if sp["over"]:
                    has, opn, lpos = False, False, 0
                else:
                    nls = [i for i, (_, t) in enumerate(ev) if t == NLc]
                    if nls:
                        has, lpos = True, base + ev[nls[-1]][0]
                        opn = not any(t >= TABc for _, t in ev[nls[-1] + 1:])
                    elif sp["cuts"]:
                        opn = False
    # the getline machine over the events: records, key ends, record ends per span, unit entries
    m, r, fs, nulf = (1 if mdbm else 0), 0, 0, False
    hdr = kHdrRecs if mdbm else 0
    keys, rec = [], {}
    units = [None] * nunit
    nu = 0
    cur, j = -1, 0
    for p, t in zip(pos.tolist(), typ.tolist()):
        while nu < nunit and nu * U <= p:
            units[nu] = dict(mode=m, r=r, nulf=nulf, fs=fs)
            nu += 1
        s = p // T
        if s != cur:
            cur, j = s, 0
        nl, nul = t == NLc, t == NULc
        brk = nl if (mdbm or m) else t == TABc
        if not nulf and (brk or nul):
            if m:
                rec.setdefault(r, [None] * 4)[2:] = [fs, p - fs]
                rec[r].append(p // U)
            else:
                keys.append(dict(r=r, fs=fs, end=p, span=s, j=j))
                rec.setdefault(r, [None] * 4)[:2] = [fs, p - fs]
        if nl and m:
            spans[s]["ends"] += 1
            r += 1
        if brk:
            fs = p + 1
        nulf = (not brk) and (nulf or nul)
        m ^= int(brk)
        j += 0 if nl else 1
    while nu < nunit:
        units[nu] = dict(mode=m, r=r, nulf=nulf, fs=fs)
        nu += 1
    count = r + m
    if m and not nulf:
        rec.setdefault(r, [None] * 4)[2:4] = [fs, n - fs]
    if mdbm and not m and fs < n:
        count += 1
        if not nulf:
            rec.setdefault(r, [None] * 4)[:2] = [fs, n - fs]
        rec[r][2:4] = rec[r - 1][2:4] if r > hdr else [fs, 0]
    count = max(count - hdr, 0)
    # ranks per unit, stored below kUnitSlots
    for u in range(nunit):
        rank = 0
        for s in range(u * SPU, min((u + 1) * SPU, nspan)):
            sl = spans[s]["slots"]
            for c in range(3):
                if sl[c] is not None:
                    sl[c] = sl[c]._replace(rank=rank)
                    rank += 1
        ss = spans[u * SPU:(u + 1) * SPU]
        ends = sum(x["ends"] for x in ss)
        units[u].update(named=rank, ends=ends, nrec=ends + 1, staged=ends + 1 <= SR,
                        max_ends=max(x["ends"] for x in ss))
    nk = [sum(min(units[u]["named"], US) for u in range(b * (B // U), min((b + 1) * (B // U), nunit)))
          for b in range(nblk)]
    # every key: hit, or miss and why
    for k in keys:
        sp = spans[k["span"]]
        L = k["end"] - k["fs"]
        k["len"] = L
        k["staged"] = units[k["span"] // SPU]["staged"]
        sl = sp["slots"][k["j"]] if k["j"] < 3 else None
        why = []
        if sp["over"]:
            why = ["over"]
        elif k["j"] >= 3:
            why = ["fourth_cut"]
        elif sl is not None and sl.len == L:
            assert sl.start == k["fs"]
            if sl.rank >= US:
                why = ["rank"]
        else:
            blk0 = k["span"] // kTThreads * B
            first = max(k["fs"] - 1, blk0) // T
            if data.find(b"\n", k["fs"], k["end"]) >= 0:
                why.append("newline_in_key")
            if L > SL:
                why.append("len")
            if k["fs"] < blk0 and k["fs"] - 1 < blk0 - kPre:
                why.append("head_beyond_pre")
            if any(spans[x]["over"] for x in range(first, k["span"])):
                why.append("over_between")
            if not why:
                why = ["other"]
        k["hit"], k["why"], k["slot"] = not why, why, sl
    return dict(size=n, fmt=fmt, error=ref_scan(data, fmt)[0], spans=spans, units=units, keys=keys, nk=nk, count=count,
                records=[tuple(rec[i][:4]) for i in range(hdr, hdr + count)] if all(
                    i in rec and None not in rec[i][:4] for i in range(hdr, hdr + count)) else None,
                rec_val_unit={i - hdr: rec[i][4] for i in rec if len(rec[i]) > 4})


def summary(model):
    """The quantities scenarios claim, from a span_model."""
    sp, un, keys = model["spans"], model["units"], model["keys"]
    q = dict(
        ev_counts={x["ne"] for x in sp},
        over_spans=sum(x["over"] for x in sp),
        over_at={s % SPU for s, x in enumerate(sp) if x["over"]},
        max_packed=max([x["ne"] for x in sp if not x["over"]], default=0),
        max_ends_in_span=max([x["ends"] for x in sp], default=0),
        ends_in_span={x["ends"] for x in sp},
        nb7=any(u["max_ends"] > 3 for u in un),
        named=[u["named"] for u in un],
        nrec=[u["nrec"] for u in un],
        staged=[u["staged"] for u in un],
        unit_modes=[u["mode"] for u in un],
        unit_nulf=[u["nulf"] for u in un],
        unit_field_back=[i * U // B - u["fs"] // B for i, u in enumerate(un)],
        nk=model["nk"],
        second_load=any(u["named"] > SPU for u in un),
        second_round=any(x > kTThreads for x in model["nk"]),
        hits=sum(k["hit"] for k in keys),
        misses=Counter(w for k in keys for w in k["why"]),
        sources={("staged" if k["staged"] else "direct", "hit" if k["hit"] else "miss") for k in keys},
        hit_kinds=Counter(k["slot"].kind for k in keys if k["hit"]),
        hit_lens={k["len"] for k in keys if k["hit"]},
        miss_lens={k["len"] for k in keys if not k["hit"]},
        hit_classes={(min(max(k["len"], 1), 128) - 1) >> 4 for k in keys if k["hit"]},
        hit_cuts={k["j"] for k in keys if k["hit"]},
        cand_only_spans=sum(1 for x in sp if x["cands"] and not x["ne"]),
        false_only_spans=sum(1 for x in sp if x["false"] and x["false"] == x["cands"]),
        false_cands=sum(x["false"] for x in sp),
        packed_full_with_false=sum(1 for x in sp if x["ne"] == EC and x["cands"] > EC),
        count=0 if model["error"] else model["count"],
        error=model["error"],
    )
    used = {id(k["slot"]) for k in keys if k["hit"]}
    q["unused_slots"] = Counter(s.kind for x in sp for s in x["slots"] if s is not None and id(s) not in used)
    # an open key whose newline lies in the block's first wave and whose end in the second
    q["open_wave_cross"] = sum(1 for k in keys if k["hit"] and k["slot"].kind == "open"
                               and (k["fs"] - 1) // U != k["end"] // U)
    q["open_span_gaps"] = {k["span"] - (k["fs"] - 1) // T for k in keys if k["slot"] is not None and k["slot"].kind == "open"
                           and k["hit"]} | {k["span"] - (k["fs"] - 1) // T for k in keys if "len" in k["why"]}
    q["rank_miss_after_stored_slot0"] = sum(
        1 for k in keys if k["why"] == ["rank"] and k["j"] >= 1 and sp[k["span"]]["slots"][0] is not None
        and sp[k["span"]]["slots"][0].rank < US)
    # records whose key ends in a unit of one store form and whose value ends in one of the other
    kv = set()
    for k in keys:
        vu = model["rec_val_unit"].get(k["r"] - (kHdrRecs if model["fmt"] == "mdbm" else 0))
        if vu is not None and vu != k["span"] // SPU:
            kv.add(("staged" if k["staged"] else "direct", "staged" if un[vu]["staged"] else "direct"))
    q["split_kv"] = kv
    return q


def claims_hold(q, claims):
    """Every claim against the summary: a plain value means equality, (">=", x) a lower bound,
    ("has", x) membership / subset, ("at", i, x) element i of a list."""
    bad = []
    for name, want in claims.items():
        got = q[name]
        if isinstance(want, tuple) and want and want[0] == ">=":
            ok = got >= want[1]
        elif isinstance(want, tuple) and want and want[0] == "has":
            need = want[1] if isinstance(want[1], (set, frozenset)) else {want[1]}
            ok = need <= set(got if not isinstance(got, Counter) else [k for k, v in got.items() if v])
        elif isinstance(want, tuple) and want and want[0] == "at":
            ok = len(got) > want[1] and got[want[1]] == want[2]
        else:
            ok = got == want
        if not ok:
            bad.append((name, want, got))
    return bad


# ------------------------------------------------------------------------------- byte helpers
def _rng(*salt):
    return np.random.default_rng([7100 + int(x) for x in salt])


def fill(n, *salt):
    """n bytes of both signs, none below 0x20."""
    return _rng(1, *salt).integers(0x20, 256, n, dtype=np.uint8).tobytes()


_LOW = np.array(list(range(1, 9)) + list(range(0x0B, 0x20)), np.uint8)


def low(n, *salt):
    """n bytes of 0x01-0x08 and 0x0B-0x1F: candidates that are no events, and false candidates."""
    return _LOW[_rng(2, *salt).integers(0, _LOW.size, n)].tobytes()


def record(klen, vlen, sep, *salt, gen=fill):
    return gen(klen, 3, *salt) + sep + gen(vlen, 4, *salt) + b"\n"


def sized(sizes, sep, *salt, klens=(8,), gen=fill):
    """Records of the given total sizes (key + delimiter + value + newline)."""
    out = []
    for i, sz in enumerate(sizes):
        kl = min(klens[i % len(klens)], sz - 2)
        out.append(record(kl, sz - 2 - kl, sep, i, *salt, gen=gen))
    return b"".join(out)


def even(nrec, total, sep, *salt, klens=(8,)):
    """nrec records that fill exactly `total` bytes: a record whose key (klens, cycled) does not
    fit the mean size gets its key + 22 bytes, the others share the rest evenly."""
    kl = [klens[i % len(klens)] for i in range(nrec)]
    mean = total // nrec
    big = {i: kl[i] + 22 for i in range(nrec) if kl[i] + 2 > mean}
    base, extra = divmod(total - sum(big.values()), nrec - len(big))
    assert base >= 2 and all(k + 2 <= base for i, k in enumerate(kl) if i not in big)
    sizes, j = [], 0
    for i in range(nrec):
        if i in big:
            sizes.append(big[i])
        else:
            sizes.append(base + (j < extra))
            j += 1
    return sized(sizes, sep, *salt, klens=klens)


ORD_MIN, ORD_MAX = T + 2, T + T // 2   # about 50 records per unit, one newline per span: nothing rare


def ordinary(nbytes, sep, *salt):
    """Exactly nbytes of whole records of ORD_MIN..ORD_MAX bytes (the last one takes what is left)."""
    assert nbytes == 0 or nbytes >= 2, nbytes
    rng = _rng(5, *salt)
    sizes = []
    left = nbytes
    while left > 3 * ORD_MIN:
        sizes.append(int(rng.integers(ORD_MIN, ORD_MAX + 1)))
        left -= sizes[-1]
    if left >= 2 * ORD_MIN:
        sizes += [left // 2, left - left // 2]
    elif left >= ORD_MIN or not sizes:
        sizes += [left] if left else []
    else:
        sizes[-1] += left
    return sized(sizes, sep, 6, *salt)


Scenario = namedtuple("Scenario", "row name data fmt claims")
SEP = {"tsv": b"\t", "mdbm": b"\n"}


# ---------------------------------------------------------------------- builders, TSV span level
def _spans_file(spans, lead=0, tail=4):
    """Three ordinary spans, an open value, `lead` more value bytes, then each pattern padded with
    value bytes to a whole span (so at lead = 0 pattern i starts at offset 0 of span 4 + i and is
    entered in mode V), the value's end and `tail` ordinary spans."""
    head = ordinary(3 * T, b"\t", 11) + fill(8, 12) + b"\t" + fill(T - 9 + lead, 13)
    body = b"".join(p + fill(T - len(p) % T if len(p) % T else 0, 14, i) for i, p in enumerate(spans))
    return head + body + b"\n" + ordinary(tail * T, b"\t", 15)


def row1_events():
    """Spans of exactly 0, 1, kEvCap - 1, kEvCap, kEvCap + 1 and 2 kEvCap events, mixed types and
    newlines only; one file with an over span first, in the middle and last in its unit."""
    out = []
    for kind in ("mixed", "nl"):
        pats = []
        for ne in (0, 1, EC - 1, EC, EC + 1, 2 * EC):
            at = np.linspace(0, T - 1, ne).astype(int) if ne > 1 else np.array([T // 2] * ne, int)
            b = bytearray(fill(T, 16, ne))
            for i, o in enumerate(at.tolist()):
                b[o] = b"\n\t\0"[(i + ne) % 3] if kind == "mixed" else 10
            pats.append(bytes(b))
        for lead in (0, 1, T - 1):
            claims = dict(ev_counts=("has", {0, 1, EC - 1, EC, EC + 1, 2 * EC}), over_spans=2, max_packed=EC) \
                if lead == 0 else dict(over_spans=(">=", 1))
            out.append(Scenario(1, f"ev-{kind}-lead{lead}", _spans_file(pats, lead), "tsv", claims))
    over = (b"\n" + fill(3, 17) + b"\t" + fill(3, 18)) * (EC // 2 + 1)
    over += fill(T - len(over), 19)
    assert len(over) == T
    u = bytearray(ordinary(U, b"\t", 20) + fill(8, 21) + b"\t" + fill(U - 9, 22) + fill(2 * U, 23) + b"\n"
                  + ordinary(T, b"\t", 24))
    for s in (2 * SPU, 2 * SPU + SPU // 2, 3 * SPU - 1):
        u[s * T:(s + 1) * T] = over
    out.append(Scenario(1, "over-first-middle-last", bytes(u), "tsv",
                        dict(over_spans=3, over_at={0, SPU // 2, SPU - 1}, misses=("has", "over"))))
    return out


def row2_record_ends():
    """A span that ends 3, 4, 63 and 64 records ("\\t\\n" pairs entered in K, "\\n" pairs "\\t"
    entered in V) and nothing else, ordinary spans before and after it in its unit."""
    out = []
    for k in (3, 4, T // 2 - 1, T // 2):
        for mode in "KV":
            pat = b"\t\n" * k if mode == "K" else b"\n" + b"\t\n" * (k - 1) + b"\t"
            for lead in ((0, 1, T - 1, T - 3) if k in (4, T // 2) else (0,)):
                start = 3 * T + lead
                if mode == "K":
                    data = ordinary(start, b"\t", 31, lead) + pat + sized([T - 2 * k + 10], b"\t", 32)
                else:
                    data = ordinary(start - 20, b"\t", 31, lead) + fill(8, 33) + b"\t" + fill(11, 34) + pat + \
                        fill(T - 2 * k + 5, 35) + b"\n"
                data += ordinary(20 * T, b"\t", 36)
                claims = dict(ends_in_span=("has", k), nb7=k > 3) if lead == 0 else dict(nb7=True) if k > 6 else {}
                if lead == 0:
                    claims["max_ends_in_span"] = k
                out.append(Scenario(2, f"ends{k}-{mode}-lead{lead}", data, "tsv", claims))
    return out


def _at_word(cur, piece_at, wo):
    """Filler length 1..4 so that cur + filler + piece_at lands on word offset wo."""
    return (wo - cur - piece_at) % 4 or 4


def row3_low_bytes():
    out = [Scenario(3, "low-records", ordinary(2 * T, b"\t", 41) + sized(
        _rng(42).integers(10, 90, 60).tolist(), b"\t", 43, klens=(1, 5, 17, 30, 60), gen=low) + ordinary(T, b"\t", 44),
        "tsv", dict(false_cands=(">=", 20)))]
    for name, wos in (("word", (0, 0, 0)), ("split", (3, 3, 2)), ("split2", (3, 3, 1)), ("split3", (2, 2, 3))):
        d = ordinary(T, b"\t", 45)
        # "\n\x0b": a value's newline, then a key that starts with 0x0B
        d += fill(_at_word(len(d), 3, wos[0]), 46) + b"\tvv" + b"\n\x0b" + fill(2, 47) + b"\t" + fill(2, 48) + b"\n"
        # "\0\x0b" inside a key
        d += fill(_at_word(len(d), 0, wos[1]), 49) + b"\0\x0b" + fill(2, 50) + b"\t" + fill(1, 51) + b"\n"
        # "\t\x0b\x0b\x0b": the key's TAB, then a value that starts with three 0x0B
        d += fill(_at_word(len(d), 0, wos[2]), 52) + b"\t\x0b\x0b\x0b" + fill(1, 53) + b"\n"
        d += ordinary(2 * T, b"\t", 54)
        want = dict(false_cands=5 if name == "word" else (">=", 1))
        out.append(Scenario(3, f"pairs-{name}", d, "tsv", want))
    # inside one long value: a span whose candidates (0x01-0x08, and the 0x0B behind each: a false
    # candidate always follows a real one in its word) are no events; a span of 0x0B bytes that no
    # borrow reaches; a span of kEvCap events plus such candidates
    quiet = bytearray(fill(T, 55))
    for o in range(8, T - 8, 8):
        quiet[o:o + 2] = bytes([1 + o % 8, 0x0B])
    falses = bytearray(fill(T, 56))
    falses[0:4] = b"\x0b\x0b\x0b\x0b"
    full = bytearray(fill(T, 57))
    evs = b"\n" + fill(2, 58) + b"\t" + fill(2, 59) + b"\n" + fill(2, 60) + b"\t" + fill(1, 61) + b"\0\x0b" + b"\t\x0b\x0b"
    assert sum(c in b"\n\t\0" for c in evs) == EC
    full[4:4 + len(evs)] = evs
    for o in range(40, T - 8, 4):
        full[o:o + 2] = bytes([1 + o % 8, 0x0B])
    for lead in (0, 1, T - 1):
        claims = dict(cand_only_spans=(">=", 1), packed_full_with_false=1, over_spans=0) if lead == 0 else {}
        out.append(Scenario(3, f"false-only-and-full-lead{lead}",
                            _spans_file([bytes(quiet), bytes(falses), bytes(full)], lead), "tsv", claims))
    return out


def row4_cuts():
    k = lambda n, s: fill(n, 70, s)   # noqa: E731
    pats = {
        "keys1": b"v\n" + k(5, 1) + b"\t" + k(3, 2),
        "keys2": b"v\n" + k(5, 3) + b"\tv\n" + k(17, 4) + b"\t" + k(3, 5),
        "keys3": b"v\n" + k(1, 6) + b"\tv\n" + k(16, 7) + b"\tv\n" + k(33, 8) + b"\t",
        "keys4-over": b"v\n" + k(1, 9) + b"\tv\n" + k(2, 10) + b"\tv\n" + k(3, 11) + b"\tv\n" + k(4, 12) + b"\t",
        "value-tabs-fourth": b"v\t\n" + k(4, 13) + b"\tv\tv\n" + k(6, 14) + b"\t",
        "three-value-tabs-fourth": b"v\t\t\t\n" + k(6, 15) + b"\t",
        "nul-cut-key": b"v\n" + k(2, 16) + b"\0" + k(3, 17) + b"\t" + k(3, 18),
        "empty-key": b"v\n\tv",
        "nul-first-key": b"v\n\0" + k(3, 19) + b"\tv",
        "nul-cut-value-then-key": b"v\0w\n" + k(7, 20) + b"\t",
    }
    want = {
        "keys1": dict(hits=(">=", 1)), "keys2": dict(hit_cuts=("has", {0, 1})), "keys3": dict(hit_cuts=("has", {0, 1, 2})),
        "keys4-over": dict(over_spans=1, misses=("has", "over")),
        "value-tabs-fourth": dict(misses=("has", "fourth_cut"), hit_cuts=("has", 1)),
        "three-value-tabs-fourth": dict(misses=("has", "fourth_cut")),
        "nul-cut-key": dict(hit_lens=("has", 2)), "empty-key": dict(hit_lens=("has", 0)),
        "nul-first-key": dict(hit_lens=("has", 0)), "nul-cut-value-then-key": dict(hit_cuts=("has", 1)),
    }
    out = [Scenario(4, n, _spans_file([p]), "tsv", want[n]) for n, p in pats.items()]
    for lead in (1, T - 1, T - 4):
        out.append(Scenario(4, f"all-lead{lead}", _spans_file(list(pats.values()), lead), "tsv", {}))
    return out


def _open_key(s, off, gap, end_off, between=b""):
    """A key that starts after a newline at offset `off` of span s and ends with a TAB at offset
    end_off of span s + gap; `between` replaces bytes in the middle of it."""
    d = bytearray(ordinary(s * T + off - 20, b"\t", 81, s) + fill(8, 82) + b"\t" + fill(11, 83) + b"\n")
    assert len(d) == s * T + off + 1
    key = bytearray(fill((s + gap) * T + end_off - len(d), 84, gap))
    if between:
        key[len(key) // 2:len(key) // 2 + len(between)] = between
    d += key + b"\t" + fill(9, 85) + b"\n" + ordinary(3 * T, b"\t", 86)
    return bytes(d)


def row5_open_key():
    out = []
    for gap, claims in ((1, dict(hit_kinds=("has", "open"), open_span_gaps=("has", 1))),
                        (2, dict(hit_kinds=("has", "open"), open_span_gaps=("has", 2))),
                        (40, dict(misses=("has", "len"), open_span_gaps=("has", 40)))):
        for s in (3, SPU + 5):
            out.append(Scenario(5, f"gap{gap}-span{s}", _open_key(s, T - 30, gap, 7), "tsv", claims))
    out.append(Scenario(5, "wave-cross", _open_key(SPU - 1, T - 40, 1, 20), "tsv", dict(open_wave_cross=(">=", 1))))
    out.append(Scenario(5, "wave-cross-gap2", _open_key(SPU - 2, T - 9, 2, 0), "tsv", dict(open_wave_cross=(">=", 1))))
    out.append(Scenario(5, "wave-cross-last-byte", _open_key(SPU - 1, T - 1, 1, 0), "tsv", dict(open_wave_cross=(">=", 1))))
    out.append(Scenario(5, "nul-between", _open_key(5, T - 30, 2, 7, b"\0"), "tsv", dict(hit_kinds=("has", "open"))))
    out.append(Scenario(5, "tab-between", _open_key(5, T - 30, 2, 7, b"\t"), "tsv", dict(hit_kinds=("has", "open"))))
    out.append(Scenario(5, "newline-between", _open_key(5, T - 30, 2, 7, b"\n"), "tsv", dict(misses=("has", "newline_in_key"))))
    out.append(Scenario(5, "over-between", _open_key(5, T - 30, 2, 7, b"\n" * (EC + 1)), "tsv",
                        dict(misses=("has", {"over_between", "newline_in_key"}))))
    out.append(Scenario(5, "wave-cross-nul-between", _open_key(SPU - 2, T - 9, 3, 0, b"\0"), "tsv", {}))
    return out


def _head_key(blk, c, d, inner=b""):
    """A key that ends with a TAB at offset c of block blk; the newline before it lies d bytes
    before the block (d = 0: the key starts the file).  `inner` replaces bytes d0 bytes back."""
    if d:
        pre = ordinary(blk * B - d - 20, b"\t", 91, c, d) + fill(8, 92) + b"\t" + fill(11, 93) + b"\n"
        assert len(pre) == blk * B - d + 1
    else:
        pre = b""
    key = fill(blk * B + c - len(pre), 94, c, d)
    return pre + key + b"\t" + fill(5, 95) + b"\n" + ordinary(2 * T, b"\t", 96), key


def row6_head_key():
    out = []
    for c in (0, 1, 17):
        for d in (kPre - 1, kPre, kPre + 1):
            data, key = _head_key(1, c, d)
            claims = dict(hit_kinds=("has", "head"), hit_lens=("has", c + d - 1)) if d <= kPre else \
                dict(misses=("has", "head_beyond_pre"), miss_lens=("has", c + d - 1))
            out.append(Scenario(6, f"block1-c{c}-d{d}", data, "tsv", claims))
    for ln in (1, 16, 17, SL, SL + 1):
        data, _ = _head_key(0, ln, 0)
        out.append(Scenario(6, f"block0-len{ln}", data, "tsv",
                            dict(hit_lens=("has", ln)) if ln <= SL else dict(misses=("has", "len"))))
    # a newline inside the head key, beyond and within kPre: no slot, or one of the wrong length
    for back in (kPre + 40, kPre // 2):
        data, key = _head_key(1, 17, 3 * kPre)
        a = bytearray(data)
        a[B - back] = 10
        out.append(Scenario(6, f"newline-in-head-{back}", bytes(a), "tsv", dict(
            misses=("has", "newline_in_key"), **(dict(unused_slots=("has", "head")) if back < kPre else {}))))
    # the block entered in mode V: its first cut is a value's TAB; a newline-less and a named form
    v = ordinary(B - 200, b"\t", 97) + fill(8, 98) + b"\t" + fill(191 + 30, 99) + b"\t" + fill(20, 100) + b"\n" + \
        ordinary(2 * T, b"\t", 101)
    out.append(Scenario(6, "enter-V-value-tab", v, "tsv", dict(unit_modes=("at", 2, 1))))
    v2 = ordinary(B - 40, b"\t", 102) + fill(8, 103) + b"\t" + fill(31 + 30, 104) + b"\t" + fill(20, 105) + b"\n" + \
        ordinary(2 * T, b"\t", 106)
    out.append(Scenario(6, "enter-V-value-tab-named", v2, "tsv", dict(unit_modes=("at", 2, 1), unused_slots=("has", "head"))))
    return out


def row7_slot_lengths():
    out = []
    for ln in (T - 1, T, T + 1, SL, SL + 1, 300):
        d = ordinary(2 * T + 50, b"\t", 111, ln) + record(ln, 6, b"\t", 112, ln) + ordinary(2 * T, b"\t", 113)
        claims = dict(hit_lens=("has", ln)) if ln <= SL else dict(miss_lens=("has", ln), misses=("has", "len"))
        out.append(Scenario(7, f"len{ln}", d, "tsv", claims))
    lens = [1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, T - 1]
    d = ordinary(T, b"\t", 114) + b"".join(record(ln, max(3, T // 2 - ln), b"\t", 115, ln) for ln in lens) + ordinary(T, b"\t", 116)
    out.append(Scenario(7, "chunk-classes", d, "tsv", dict(hit_classes=set(range(8)))))
    return out


# --------------------------------------------------------------- builders, TSV unit and block level
def row8_named_per_unit():
    out = []
    for i, nn in enumerate((SPU - 1, SPU, SPU + 1, SR, US - 1, US, US + 1)):
        d = ordinary(U, b"\t", 121) + even(nn, U, b"\t", 122, nn) + even(SPU // 2, U, b"\t", 123) if i % 2 else \
            even(nn, U, b"\t", 122, nn) + ordinary(U + T, b"\t", 121)
        u = 1 if i % 2 else 0
        claims = dict(named=("at", u, nn), second_load=nn > SPU)
        if nn > US:
            claims.update(misses=("has", "rank"), rank_miss_after_stored_slot0=(">=", 1))
        out.append(Scenario(8, f"named{nn}-unit{u}", d, "tsv", claims))
    # ~1.5 kUnitSlots: the smallest uniform record that keeps every span packed (<= 3 records a span)
    size = T // 3 + 1
    d = sized([size] * (3 * B // size), b"\t", 124)
    out.append(Scenario(8, "named-1.5x", d, "tsv", dict(over_spans=0, misses=("has", "rank"), second_load=True)))
    return out


def row9_records_per_unit():
    """nrec = kStageRecs - 1, kStageRecs, kStageRecs + 1 in the first and in the second unit of a
    block, every key a hit and with keys over kSpecLenMax mixed in; with a first record of 12
    bytes every unit edge falls in a value, so a record's key lies in the unit before its value's
    end (staged -> direct and direct -> staged)."""
    out = []
    for nrec in (SR - 1, SR, SR + 1):
        for u in (0, 1):
            for mix in ("hits", "misses"):
                skew = 12 if nrec > SR or (nrec + u) % 2 else 0
                kl = (8,) if mix == "hits" else (8, 8, 8, SL + 46, 8, 20, 8)
                units = [even(SPU // 2, U, b"\t", 131, j, klens=kl) for j in range(3)]
                units[u] = even(nrec - 1, U, b"\t", 132, nrec, klens=kl)
                data = (sized([skew], b"\t", 133) if skew else b"") + b"".join(units)
                claims = dict(nrec=("at", u, nrec), staged=("at", u, nrec <= SR))
                if mix == "misses":
                    claims["misses"] = ("has", "len")
                    claims["sources"] = ("has", {("staged", "miss"), ("staged", "hit")} | (
                        {("direct", "miss"), ("direct", "hit")} if nrec > SR else set()))
                if skew and nrec > SR:
                    claims["split_kv"] = ("has", {("staged", "direct"), ("direct", "staged")} if u == 1 else {("direct", "staged")})
                out.append(Scenario(9, f"nrec{nrec}-unit{u}-{mix}", data, "tsv", claims))
    return out


def row10_keys_per_block():
    out = []
    kl = (1, 16, 17, 33, 49, 65, 81, 97, 113, 120, 8)
    for nk in (0, 1, kTThreads - 1, kTThreads, kTThreads + 1, 2 * US):
        if nk == 0:      # the block lies inside one value
            data = ordinary(B - 100, b"\t", 141) + fill(8, 142) + b"\t" + fill(B + 150, 143) + b"\n" + ordinary(T, b"\t", 144)
        elif nk == 1:
            data = ordinary(B - 100, b"\t", 141) + fill(8, 142) + b"\t" + fill(91 + 100, 143) + b"\n" + \
                fill(30, 145) + b"\t" + fill(B - 100 - 32, 146) + fill(60, 147) + b"\n" + ordinary(T, b"\t", 144)
        else:
            data = ordinary(B, b"\t", 141) + even(nk, B, b"\t", 148, nk, klens=kl if nk < 2 * US else (8, 1, 16, 17, 33, 49)) + \
                ordinary(T, b"\t", 144)
        claims = dict(nk=("at", 1, nk), second_round=nk > kTThreads)
        if kTThreads - 1 <= nk <= kTThreads + 1:
            claims["hit_classes"] = set(range(8))
        out.append(Scenario(10, f"nk{nk}", data, "tsv", claims))
    d = sized([T // 3 + 1] * (2 * B // (T // 3 + 1)), b"\t", 149)
    out.append(Scenario(10, "nk-most", d, "tsv", dict(nk=("at", 0, 2 * US), second_round=True)))
    return out


def row11_block_entry():
    big = 3 * B + T   # the field starts in block 0 and ends in block 3
    out = []
    v = fill(big, 151)
    for name, val in (("V", v), ("V-nul", v[:5] + b"\0" + v[6:])):
        d = ordinary(T + 9, b"\t", 152) + fill(8, 153) + b"\t" + val + b"\n" + ordinary(2 * T, b"\t", 154)
        out.append(Scenario(11, f"enter-{name}-3blocks", d, "tsv", dict(
            unit_modes=("has", 1), unit_field_back=("has", {1, 2, 3}), unit_nulf=("has", name == "V-nul"))))
    k = bytearray(fill(big, 155))
    for o in range(100, big, 997):
        k[o] = 10
    for name, key in (("K", bytes(k)), ("K-nul", bytes(k[:7]) + b"\0" + bytes(k[8:]))):
        d = ordinary(T + 9, b"\t", 156) + key + b"\t" + fill(20, 157) + b"\n" + ordinary(2 * T, b"\t", 158)
        out.append(Scenario(11, f"enter-{name}-3blocks", d, "tsv", dict(
            unit_field_back=("has", {1, 2, 3}), unit_nulf=("has", name == "K-nul"))))
    return out


# --------------------------------------------------------------------------------- builders, EOF
EOF_TAILS = {
    "key-bytes": b"keyb", "after-newline": b"", "after-delimiter": b"kk\t", "mid-value": b"kk\tvv",
    "nul-cut-value": b"kk\tv\0w", "nul-cut-key": b"k\0y",
}
EOF_SIZES = tuple(b + e for b in (T, U, B) for e in (-1, 0, 1))
TINY = {"tsv": (b"k", b"\t", b"\n", b"\0", b"k\t", b"\t\n", b"\tv", b"\t\0", b"k\tv", b"\t\n\t", b"\0\tv", b"k\t\n", b"\n\t\n"),
        "mdbm": (b"H", b"\n\n", b"\n\n\n")}


def row12_eof(fmt):
    out = []
    sep = SEP[fmt]
    hdr = HDR74 if fmt == "mdbm" else b""
    for state, tail in EOF_TAILS.items():
        tail = tail.replace(b"\t", sep)
        for size in EOF_SIZES:
            body = size - len(hdr) - len(tail)
            d = hdr + ordinary(body, sep, 161, size) + tail
            assert len(d) == size
            out.append(Scenario(12, f"{fmt}-{state}-{size}", d, fmt, dict(count=(">=", 1))))
    for i, d in enumerate(TINY[fmt]):
        out.append(Scenario(12, f"{fmt}-tiny{i}", d, fmt, {}))
    if fmt == "mdbm":
        for state, tail in EOF_TAILS.items():
            out.append(Scenario(12, f"mdbm-{state}-bare", HDR74 + tail.replace(b"\t", b"\n"), fmt, {}))
    return out


# -------------------------------------------------------------------------------- builders, mdbm
def _header(end_at, lines=(b"format=print", b"type=btree", b"mdbm_pagesize=4096")):
    """Four header lines, the fourth padded so that HEADER=END starts at byte end_at."""
    h = b"".join(x + b"\n" for x in lines)
    return h + fill(end_at - len(h) - 1, 171, end_at) + b"\n"


def row13_header():
    out = []
    body = ordinary(3 * T, b"\n", 172)
    for name, at in (("span", T - 5), ("unit", U - 5), ("block", B - 5), ("in-block2", 2 * B + 100)):
        h = _header(at)
        out.append(Scenario(13, f"end-straddles-{name}", h + END + b"\n" + body, "mdbm", dict(count=(">=", 2))))
    h = _header(U - 5, (b"for\0mat\t=print", b"\0", b"\t\tx\0\0y"))
    out.append(Scenario(13, "nuls-tabs-in-header", h + END + b"\n" + body, "mdbm", dict(count=(">=", 2))))
    for name, l4 in (("nul", END + b"\0x"), ("short", END[:-1]), ("space", END + b" "), ("prefix", b"x" + END)):
        for at in (T // 2, U - 5):
            out.append(Scenario(13, f"bad-{name}-{at}", _header(at) + l4 + b"\n" + body, "mdbm", dict(count=0)))
    out.append(Scenario(13, "ends-in-line3", _header(U + 50)[:-1], "mdbm", dict(count=0)))
    out.append(Scenario(13, "ends-in-line1", b"format=print\ntype", "mdbm", dict(count=0)))
    out.append(Scenario(13, "end-at-eof", _header(B - 5) + END, "mdbm", dict(count=0)))
    out.append(Scenario(13, "end-at-eof-short", b"a\nb\nc\nd\n" + END, "mdbm", dict(count=0)))
    over = b"a\0\0\0\0\nb\0\nc\nd\n" + END + b"\n"
    out.append(Scenario(13, "over-span-in-header", over + body, "mdbm", dict(over_spans=(">=", 1), count=(">=", 2))))
    h = b"\n" * (EC + 2)   # more newlines than a packed span holds, four of them header lines: line 4 is empty
    out.append(Scenario(13, "over-newlines-bad", h + END + b"\n" + body, "mdbm", dict(count=0, over_spans=(">=", 1))))
    return out


def row14_lines():
    out = []
    d = HDR74 + b"k\tey\tv\tal\n\tv\n" + b"ke\0y\nva\0l\n" + b"\nv\n" + b"k\n\n" + b"\n\n" + b"\0\n\0\n" + ordinary(T, b"\n", 181)
    out.append(Scenario(14, "tabs-nuls-empties", d, "mdbm", dict(count=(">=", 7))))
    for k in (4, T // 2 - 1, T // 2):
        for lead in (0, 1):
            pre = HDR74 + ordinary(3 * T - len(HDR74) + lead, b"\n", 182)
            d = pre + b"\n\n" * k + ordinary(6 * T, b"\n", 183)
            out.append(Scenario(14, f"ends{k}-lead{lead}", d, "mdbm",
                                dict(max_ends_in_span=k, nb7=True) if lead == 0 else dict(nb7=True)))
    for nrec in (SR - 1, SR, SR + 1, 2 * SR):
        d = HDR74 + ordinary(U - len(HDR74), b"\n", 184) + even(nrec - 1, U, b"\n", 185, nrec) + ordinary(T, b"\n", 186)
        out.append(Scenario(14, f"nrec{nrec}", d, "mdbm", dict(nrec=("at", 1, nrec), staged=("at", 1, nrec <= SR))))
    # the header's unit itself direct: more than kStageRecs records after a short header
    d = HDR74 + even(2 * SR, U - len(HDR74), b"\n", 187) + ordinary(T, b"\n", 188)
    out.append(Scenario(14, "direct-header-unit", d, "mdbm", dict(staged=("at", 0, False))))
    return out


def row15_key_line_at_eof():
    """(scenario, caps) pairs: the key line at EOF, cap = count + 1, count, count - 1, 0."""
    out = []
    rec1 = b"key1\nvalue1\n"
    many = ordinary(3 * U, b"\n", 191)
    files = {
        "only": HDR74 + b"lastkey",
        "only-long-header": _header(U - 5) + END + b"\n" + b"lastkey",
        "after-one": HDR74 + rec1 + b"lastkey",
        "after-many": HDR74 + many + b"lastkey",
        "after-many-direct": HDR74 + even(3 * SR, U, b"\n", 192) + b"lastkey",
        "value-other-unit": HDR74 + rec1 + fill(U, 193),
        "value-other-block": HDR74 + many[:200] + fill(B + 100, 194),
        "value-empty": HDR74 + b"key1\n\n" + b"lastkey",
        "value-nul-cut": HDR74 + b"key1\nva\0lue\n" + b"lastkey",
        "key-nul-cut": HDR74 + rec1 + b"la\0stkey",
        "value-empty-other-unit": HDR74 + many + b"k\n\n" + fill(U + 3, 195),
    }
    for name, d in files.items():
        out.append(Scenario(15, name, d, "mdbm", dict(count=(">=", 1))))
    return out


def all_scenarios():
    s = (row1_events() + row2_record_ends() + row3_low_bytes() + row4_cuts() + row5_open_key() + row6_head_key()
         + row7_slot_lengths() + row8_named_per_unit() + row9_records_per_unit() + row10_keys_per_block()
         + row11_block_entry() + row12_eof("tsv") + row12_eof("mdbm") + row13_header() + row14_lines()
         + row15_key_line_at_eof())
    assert len({(x.row, x.name) for x in s}) == len(s)
    return s


ALL_ARM_ROWS = (1, 2, 3, 4, 5, 6, 7, 12)
STD_FNV_ROWS = {7: "tsv", 14: "mdbm"}   # one row per format also runs the std-FNV arm


def matrix(scen, index):
    """The (arm, shift, canary, cap, std_fnv) runs of one scenario; cap None = the exact count,
    otherwise an offset from it ("-1", "+1") or an absolute value."""
    runs = []
    if scen.row in ALL_ARM_ROWS:
        other = SHIFTS[1 + index % 2]
        ca, cb = CANARIES[index % 4], CANARIES[(index + 1 + index // 4 % 3) % 4]
        for arm in ARMS:
            runs += [(arm, 0, ca, None, False), (arm, other, cb, None, False)]
    else:
        shift, can = SHIFTS[index % 3], CANARIES[index % 4]
        runs += [("fused", shift, can, None, False), ("scan", shift, can, None, False)]
    if scen.row in (1, 9, 12):
        shift, can = SHIFTS[(index + 1) % 3], CANARIES[(index + 2) % 4]
        for arm in ("fused", "scan"):
            runs += [(arm, shift, can, "-1", False), (arm, shift, can, 1, False)]
    if scen.row == 13 and scen.name.startswith(("bad-", "ends-in", "over-newlines")):
        runs.append(("count", SHIFTS[index % 3], CANARIES[(index + 1) % 4], None, False))
    if scen.row == 15:
        shift, can = SHIFTS[(index + 1) % 3], CANARIES[(index + 2) % 4]
        for arm in ("fused", "scan", "fused-h1"):
            runs += [(arm, shift, can, c, False) for c in ("+1", "-1", 0)]
    if scen.row in STD_FNV_ROWS:
        runs += [("fused", 1, 0x0A, None, True), ("scan+prehash", 15, 0x00, None, True)]
    return runs


# ---------------------------------------------------------------------------------- device side
def place(cuda, payload, shift, canary):
    """The file as a device buffer that starts `shift` bytes into a 128-aligned place of its
    allocation and ends at the file's last byte, PAD canary bytes before (plus the shift) and after."""
    import torch
    a = np.full(PAD + shift + len(payload) + PAD, canary, np.uint8)
    a[PAD + shift:PAD + shift + len(payload)] = np.frombuffer(payload, np.uint8)
    t = torch.from_numpy(a).to(cuda)
    assert t.data_ptr() % 128 == 0, "device allocations are expected 128-aligned"
    return t[PAD + shift:PAD + shift + len(payload)]


def run_scan(cuda, file, fmt, arm, cap, std_fnv=False):
    """One arm of the C ABI over the device file into sentinel-filled outputs of cap + GUARD rows:
    (rc, count, dict of host arrays recs (rows, 4) / h1 / h2)."""
    import torch

    from k2hash_amd import _native
    from k2hash_amd.batch import _stream_handle
    lib = _native.batch_lib()
    code = {"tsv": _native.K2H_AMD_IMPORT_TSV, "mdbm": _native.K2H_AMD_IMPORT_MDBM}[fmt]
    flags = _native.K2H_AMD_FLAG_STD_FNV if std_fnv else 0
    rows = cap + GUARD
    recs = torch.full((rows, 4), SENTINEL, dtype=torch.int64, device=cuda)
    h1 = torch.full((rows,), SENTINEL, dtype=torch.int64, device=cuda)
    h2 = torch.full((rows,), SENTINEL, dtype=torch.int64, device=cuda)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    fp = ctypes.c_void_p(file.data_ptr() or 1)
    cnt = ctypes.c_uint64(0xDEAD)
    st = _stream_handle(None)
    if arm == "count":
        rc = lib.k2h_amd_import_scan_device(fp, file.numel(), code, None, 0, ctypes.byref(cnt), st)
    elif arm in ("scan", "scan+prehash"):
        rc = lib.k2h_amd_import_scan_device(fp, file.numel(), code, ptr(recs), cap, ctypes.byref(cnt), st)
        if arm == "scan+prehash" and rc == 0:
            rc = lib.k2h_amd_import_prehash(fp, file.numel(), ptr(recs), min(cnt.value, cap), ptr(h1), ptr(h2), flags, st)
    else:
        rc = lib.k2h_amd_import_scan_prehash_device(fp, file.numel(), code, ptr(recs), cap, ctypes.byref(cnt), ptr(h1),
                                                    None if arm == "fused-h1" else ptr(h2), flags, st)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().view(np.uint64) for k, v in (("recs", recs), ("h1", h1), ("h2", h2))}
    return rc, cnt.value, got


def check(what, arm, cap, rc, count, got, error, want_recs, want_h1, want_h2):
    """The contract of every arm."""
    sent = np.uint64(SENTINEL)
    n_ref = 0 if error else len(want_recs)
    gives_recs = arm != "count"
    assert rc == (EINVAL if error or (gives_recs and n_ref > cap) else 0), (what, "rc", rc)
    assert count == n_ref, (what, "count", count, n_ref)
    n = min(n_ref, cap) if gives_recs else 0
    want = recs_array(want_recs[:n])
    names = ("key_off", "key_len", "val_off", "val_len")
    for c in range(4):
        bad = np.flatnonzero(got["recs"][:n, c] != want[:, c])
        assert bad.size == 0, (what, names[c], f"{bad.size} of {n} rows differ, first row {int(bad[0])}: "
                               f"{int(got['recs'][bad[0], c])} != {int(want[bad[0], c])}")
    assert (got["recs"][n:] == sent).all(), (what, "recs written at or past row", n)
    nh = {"scan": 0, "count": 0}.get(arm, n)
    for name, ref, rows in (("h1", want_h1, nh), ("h2", want_h2, 0 if arm == "fused-h1" else nh)):
        bad = np.flatnonzero(got[name][:rows] != ref[:rows])
        assert bad.size == 0, (what, name, f"{bad.size} of {rows} differ, first at record {int(bad[0])}: "
                               f"{int(got[name][bad[0]]):#x} != {int(ref[bad[0]]):#x}")
        assert (got[name][rows:] == sent).all(), (what, name, "written at or past row", rows)
