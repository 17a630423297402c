#!/usr/bin/env python3
"""LDS bank-conflict model of the split-exchange (one float per element) Stockham transform.

Banking per MI355X_MICROARCH.md §LDS: ds_read_b32 / ds_write_b32 are serviced in two 32-lane
groups, bank = dword address mod 32; a group costs (max distinct addresses on one bank) cycles.
Evaluates a padding function over every exchange of the power-of-two schedule.
usage: lds_bank_sim.py [N] [T]   |   lds_bank_sim.py layouts
       lds_bank_sim.py pairs | pairs-search   (the two-line image under the 8-byte rules)"""
import sys

import numpy as np


def sched(n, v=16, small_first=False):
    lg = n.bit_length() - 1
    lv = v.bit_length() - 1
    rad = [v] * (lg // lv)
    rem = 1 << (lg % lv)
    if rem > 1:
        rad = ([rem] + rad) if small_first else (rad + [rem])
    return rad


def group_cycles(addr):
    """addr: [64] dword addresses of one wave-instruction -> LDS cycles (2 groups of 32)."""
    cyc = 0
    for g in (addr[:32], addr[32:]):
        banks = {}
        for a in set(int(x) for x in g):
            banks.setdefault(a % 32, set()).add(a)
        cyc += max(len(s) for s in banks.values())
    return cyc


def exchange_cost(n, t, pad, small_first=False):
    rad = sched(n, 16 if n // 16 <= 1024 else 16, small_first)
    L = 1
    tot = ideal = 0
    tid = np.arange(t)
    for s in range(len(rad) - 1):
        R, R2 = rad[s], rad[s + 1]
        NB, NB2 = n // R, n // R2
        MB, MB2 = NB // t, NB2 // t
        # writes: output j = (i - k) R + k + r L
        for m in range(MB):
            i = tid + m * t
            k = i & (L - 1)
            for r in range(R):
                a = pad((i - k) * R + k + r * L)
                for w in range(t // 64):
                    c = group_cycles(a[64 * w:64 * w + 64]); tot += c; ideal += 2
        # reads of the next stage: i2 + r2 NB2
        for m in range(MB2):
            i2 = tid + m * t
            for r in range(R2):
                a = pad(i2 + r * NB2)
                for w in range(t // 64):
                    c = group_cycles(a[64 * w:64 * w + 64]); tot += c; ideal += 2
        L *= R
    return tot, ideal


PADS = {
    "j+j>>4 (current)": lambda j: j + (j >> 4),
    "j+j>>5": lambda j: j + (j >> 5),
    "j+j>>5+j>>9": lambda j: j + (j >> 5) + (j >> 9),
    "j+j>>4+j>>8": lambda j: j + (j >> 4) + (j >> 8),
    "xor(j>>5)": lambda j: j ^ ((j >> 5) & 31),
    "xor(j>>4)": lambda j: j ^ ((j >> 4) & 31),
    "xor(j>>5)^(j>>10)": lambda j: j ^ (((j >> 5) ^ (j >> 10)) & 31),
    "none": lambda j: j,
}

def report():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    t = int(sys.argv[2]) if len(sys.argv) > 2 else n // 16
    for sf in (False, True):
        print("N", n, "T", t, "small_first", sf, "schedule", sched(n, 16, sf))
        for name, f in PADS.items():
            tot, ideal = exchange_cost(n, t, f, sf)
            print(f"  {name:22s} cycles {tot:7d}  ideal {ideal:7d}  extra {100.0 * (tot - ideal) / ideal:6.1f} %")


def search(n=8192, t=None):
    """Additive paddings j + (j >> a) [+ (j >> b)]: extra bank cycles for both schedules."""
    t = t or n // 16
    res = []
    for a in range(3, 10):
        for b in [None] + list(range(a + 1, 13)):
            f = (lambda j, a=a, b=b: j + (j >> a) + ((j >> b) if b else 0))
            c0, i0 = exchange_cost(n, t, f, False)
            c1, i1 = exchange_cost(n, t, f, True)
            res.append(((c0 - i0) / i0, (c1 - i1) / i1, a, b or 0, int(f(np.array([n - 1]))[0]) + 1))
    res.sort()
    for r in res[:12]:
        print("  pad j+(j>>%d)%s: extra %.1f %% / %.1f %% (small-first), footprint %d floats" %
              (r[2], (" + (j>>%d)" % r[3]) if r[3] else "", 100 * r[0], 100 * r[1], r[4]))


def per_site(n, t, pad, small_first=False):
    rad = sched(n, 16, small_first)
    L = 1
    tid = np.arange(t)
    out = []
    for s in range(len(rad) - 1):
        R, R2 = rad[s], rad[s + 1]
        NB, NB2 = n // R, n // R2
        for kind, MB_, RR, fn in (("write", NB // t, R, lambda i, r: (i - (i & (L - 1))) * R + (i & (L - 1)) + r * L),
                                  ("read", NB2 // t, R2, lambda i, r: i + r * NB2)):
            tot = ideal = 0
            for m in range(MB_):
                i = tid + m * t
                for r in range(RR):
                    a = pad(fn(i, r))
                    for w in range(t // 64):
                        tot += group_cycles(a[64 * w:64 * w + 64]); ideal += 2
            out.append((s, kind, L, R, tot / ideal))
        L *= R
    return out


def sites(n, t, small_first):
    """Per exchange e: list of (kind, [lane-index arrays per r]) of the write and the next read."""
    rad = sched(n, 16, small_first)
    L = 1
    tid = np.arange(t)
    ex = []
    for s in range(len(rad) - 1):
        R, R2 = rad[s], rad[s + 1]
        NB, NB2 = n // R, n // R2
        w = [[(i - (i & (L - 1))) * R + (i & (L - 1)) + r * L for r in range(R)]
             for i in (tid + m * t for m in range(NB // t))]
        rd = [[i + r * NB2 for r in range(R2)] for i in (tid + m * t for m in range(NB2 // t))]
        ex.append((L, R, w, rd))
        L *= R
    return ex


def best_layouts(n, small_first):
    t = n // 16
    out = []
    for L, R, w, rd in sites(n, t, small_first):
        best = None
        for sh in range(3, 12):
            for c in (1, 2, 4, 8, 16):
                f = lambda j, sh=sh, c=c: j + c * (j >> sh)
                foot = int(f(n - 1)) + 1
                if foot > n + n // 16:
                    continue
                ok = True   # constant-offset addressing: f(j_r) - f(j_0) lane-independent
                cyc = ideal = 0
                for grp in (w, rd):
                    for per_m in grp:
                        base = f(per_m[0])
                        for jr in per_m:
                            d = f(jr) - base
                            ok &= bool(np.all(d == d[0]))
                            a = f(jr)
                            for wv in range(t // 64):
                                cyc += group_cycles(a[64 * wv:64 * wv + 64]); ideal += 2
                if not ok:
                    continue
                key = (cyc / ideal, foot)
                if best is None or key < best[0]:
                    best = (key, sh, c)
        out.append((L, R, best[1], best[2], round(best[0][0], 3), best[0][1]))
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("layouts64", "pairs", "pairs-search"):
        pass  # below
    elif len(sys.argv) > 1 and sys.argv[1] == "layouts":
        for n in (1024, 2048, 4096, 8192, 16384):
            for sf in (False, True):
                print(n, "small_first" if sf else "radix16_first", best_layouts(n, sf))
    else:
        report()


def cyc_b64_read(p):
    """ds_read_b64 of complex elements at float2 index p: 2 x 32 lanes, bank = dword mod 64."""
    cyc = 0
    for g in (p[:32], p[32:]):
        banks = {}
        for e in set(int(x) for x in g):
            for d in (2 * e, 2 * e + 1):
                banks.setdefault(d % 64, set()).add(d)
        cyc += max(len(s) for s in banks.values())
    return cyc


def cyc_b64_write(p):
    """ds_write_b64: 4 x 16 contiguous lanes, bank = dword mod 32."""
    cyc = 0
    for q in range(4):
        g = p[16 * q:16 * q + 16]
        banks = {}
        for e in set(int(x) for x in g):
            for d in (2 * e, 2 * e + 1):
                banks.setdefault(d % 32, set()).add(d)
        cyc += max(len(s) for s in banks.values())
    return cyc


def best_layouts_c64(n, small_first, verbose=False):
    """Complex (float2) image: per exchange, the additive layout with the fewest LDS cycles."""
    t = n // 16
    out = []
    for L, R, w, rd in sites(n, t, small_first):
        res = []
        for sh in range(2, 12):
            for c in (0, 1, 2, 4, 8, 16):
                if c == 0 and sh > 2:
                    continue
                f = lambda j, sh=sh, c=c: j + c * (j >> sh)
                foot = int(f(n - 1)) + 1
                if foot > n + n // 16 + 1:
                    continue
                ok = True
                cyc = ideal = 0
                for grp, cf, idl in ((w, cyc_b64_write, 4), (rd, cyc_b64_read, 2)):
                    for per_m in grp:
                        base = f(per_m[0])
                        for jr in per_m:
                            d = f(jr) - base
                            ok &= bool(np.all(d == d[0]))
                            a = f(jr)
                            for wv in range(t // 64):
                                cyc += cf(a[64 * wv:64 * wv + 64]); ideal += idl
                if ok:
                    res.append((cyc / ideal, foot, sh, c))
        res.sort()
        cur = [r for r in res if r[2] == 4 and r[3] == 1]
        out.append((L, R, res[0][2], res[0][3], round(res[0][0], 3), "current", round(cur[0][0], 3) if cur else None))
    return out


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "layouts64":
    for n in (1024, 2048, 4096, 8192, 16384):
        for sf in (False, True):
            print(n, "small_first" if sf else "radix16_first", best_layouts_c64(n, sf))


# ---------------------------------------------------------------------------------------------
# Two-line (row pair) exchange: element j of the image is one float2 {line 0, line 1} at float2
# index lay(j), moved by ds_write_b64 / ds_read_b64 (rules of MI355X_MICROARCH.md §LDS, as
# cyc_b64_write / cyc_b64_read above: stores in 4 x 16 contiguous lanes over 32 dword banks, loads
# in 2 x 32 lanes over 64 dword banks).  split_lay / pair_lay mirror csrc/thz_fft.hpp.
# ---------------------------------------------------------------------------------------------
PAIR_SIZES = (1024, 2048, 4096, 8192, 16384)


def split_lay(L, j):
    sh, c = (5, 1) if L == 1 else ((3 + L.bit_length(), L) if L <= 16 else (11, 1))
    return j + c * (j >> sh)


def pair_lay(L, j):
    if L == 1:
        return 34 * (j >> 5) + 2 * (j & 15) + ((j >> 4) & 1)
    if L == 256:
        return j + (j >> 9)
    return split_lay(L, j)


def pair_image_f2(n):
    """float2 slots of the pair image (2 lds_split_f2(n) of csrc/thz_fft.hpp)."""
    return 2 * ((n + (n >> 4) + 1 + 1) // 2)


def pair_exchange_table(n, lay=pair_lay):
    """Per exchange of the row schedule (radix 16 first, T = n / 16) under the b64 rules:
    dict(L, R, R2, st_cyc, st_ideal, ld_cyc, ld_ideal, const_offsets, footprint)."""
    t = n // 16
    rows = []
    for L, R, w, rd in sites(n, t, False):
        f = lambda j, L=L: lay(L, j)
        row = dict(L=L, R=R, R2=len(rd[0]), const_offsets=True,
                   footprint=int(f(np.array([n - 1]))[0]) + 1)
        for key, grp, cf, idl in (("st", w, cyc_b64_write, 4), ("ld", rd, cyc_b64_read, 2)):
            cyc = ideal = 0
            for per_m in grp:
                base = f(per_m[0])
                for jr in per_m:
                    a = f(jr)
                    d = a - base
                    row["const_offsets"] &= bool(np.all(d == d[0]))
                    for wv in range(t // 64):
                        cyc += cf(a[64 * wv:64 * wv + 64]); ideal += idl
            row[key + "_cyc"], row[key + "_ideal"] = cyc, ideal
        rows.append(row)
    return rows


def search_pair_layouts(n):
    """Per exchange: the conflict-free layouts among j + c (j >> sh) and the half-interleaved blocks
    (2^b + c) (j >> b) + 2 (j & (2^(b-1) - 1)) + ((j >> (b-1)) & 1) that keep constant r-offsets and
    fit the image; returns {L: [names]}."""
    cands = {}
    for sh in range(3, 12):
        for c in (1, 2, 4, 8, 16):
            cands["j+%d*(j>>%d)" % (c, sh)] = lambda L, j, sh=sh, c=c: j + c * (j >> sh)
    for b in (4, 5, 6):
        for c in (0, 1, 2, 4):
            cands["%d*(j>>%d)+2*(j&%d)+((j>>%d)&1)" % ((1 << b) + c, b, (1 << (b - 1)) - 1, b - 1)] = \
                lambda L, j, b=b, c=c: ((1 << b) + c) * (j >> b) + 2 * (j & ((1 << (b - 1)) - 1)) + ((j >> (b - 1)) & 1)
    out = {}
    for name, f in cands.items():
        for row in pair_exchange_table(n, f):
            if (row["const_offsets"] and row["footprint"] <= pair_image_f2(n) and row["st_cyc"] == row["st_ideal"]
                    and row["ld_cyc"] == row["ld_ideal"]):
                out.setdefault(row["L"], []).append(name)
    return out


def pairs_report():
    print("two-line exchange under the b64 rules: LDS-array cycles / conflict-free cycles per workgroup")
    print("%6s %5s %3s %3s | %-19s %-19s | %-19s %-19s %s" % ("N", "L", "R", "R2", "split_lay store", "split_lay load",
                                                             "pair_lay store", "pair_lay load", "offsets footprint/image"))
    for n in PAIR_SIZES:
        for old, new in zip(pair_exchange_table(n, split_lay), pair_exchange_table(n)):
            print("%6d %5d %3d %3d | %8d / %-8d %8d / %-8d | %8d / %-8d %8d / %-8d %s %d/%d" % (
                n, new["L"], new["R"], new["R2"], old["st_cyc"], old["st_ideal"], old["ld_cyc"], old["ld_ideal"],
                new["st_cyc"], new["st_ideal"], new["ld_cyc"], new["ld_ideal"],
                "const" if new["const_offsets"] else "PER-LANE", new["footprint"], pair_image_f2(n)))


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "pairs":
    pairs_report()
if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "pairs-search":
    for n in PAIR_SIZES:
        for L, names in sorted(search_pair_layouts(n).items()):
            print(n, "L", L, "conflict-free:", ", ".join(names))
