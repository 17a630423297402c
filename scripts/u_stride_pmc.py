#!/usr/bin/env python3
"""Per-channel L2 counters of the ASM column pass (K2) and inverse row pass (K3) from rocprofv3's
JSON output.

usage: scripts/u_stride_pmc.py OUT.json LABEL=DIR[,DIR...] [LABEL=DIR...]

Each DIR holds the run_results.json of one `rocprofv3 --pmc ... --output-format json -- python3
bench.py --steps 3` run (counters only, one run per counter group).  The JSON keeps one value per
counter instance -- for the TCC block one per L2 channel (8 XCDs x 16 channels) -- where the CSV
holds their sum.  For every kernel of a label and every counter: the sum over the channels and the
max / mean ratio over them, averaged over the kernel's launches; then the stall shares
TCC_EA0_WRREQ_STALL / TCC_CYCLE, TCC_TAG_STALL / TCC_CYCLE and TCC_BUSY / TCC_CYCLE where the
run collected both sides.
"""
import collections
import json
import os
import sys

KERNELS = {"asm_cols<": "K2", "asm_rows_inv": "K3", "asm_rows_fwd<": "K1"}


def one_run(path):
    """{kernel tag: {counter: [per-instance values averaged over launches]}}"""
    tool = json.load(open(path))["rocprofiler-sdk-tool"][0]
    cname = {c["id"]["handle"]: c["name"] for c in tool["counters"]}
    kname = {k["kernel_id"]: k.get("formatted_kernel_name") or k.get("demangled_kernel_name") or k["kernel_name"]
             for k in tool["kernel_symbols"]}
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for rec in tool["callback_records"]["counter_collection"]:
        name = kname.get(rec["dispatch_data"]["dispatch_info"]["kernel_id"], "")
        tag = next((t for s, t in KERNELS.items() if "thz::" + s in name), None)
        if tag is None:
            continue
        inst = collections.defaultdict(list)
        for r in rec["records"]:
            inst[cname[r["counter_id"]["handle"]]].append(float(r["value"]))
        for c, v in inst.items():
            acc[tag][c].append(v)
    out = {}
    for tag, d in acc.items():
        out[tag] = {}
        for c, launches in d.items():
            n = min(len(v) for v in launches)
            out[tag][c] = [sum(v[i] for v in launches) / len(launches) for i in range(n)]
    return out


def summarise(dirs):
    per = collections.defaultdict(dict)
    for d in dirs:
        for tag, cs in one_run(os.path.join(d, "run_results.json")).items():
            per[tag].update(cs)
    res = {}
    for tag, cs in sorted(per.items()):
        r = {}
        for c, v in sorted(cs.items()):
            s = sum(v)
            r[c] = {"instances": len(v), "sum": s, "max_over_mean": (max(v) * len(v) / s) if s else None}
        cyc = r.get("TCC_CYCLE", {}).get("sum")
        for c in ("TCC_EA0_WRREQ_STALL", "TCC_TAG_STALL", "TCC_BUSY", "TCC_EA0_RDREQ_DRAM_CREDIT_STALL"):
            if cyc and c in r:
                r[c + "_per_TCC_CYCLE"] = r[c]["sum"] / cyc
        res[tag] = r
    return res


def main():
    out = {}
    for arg in sys.argv[2:]:
        label, dirs = arg.split("=", 1)
        out[label] = summarise(dirs.split(","))
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
    for label, ks in out.items():
        for tag, r in ks.items():
            for c, v in r.items():
                if isinstance(v, dict):
                    print(f"{label:8s} {tag} {c:34s} sum {v['sum']:.4g}  max/mean {v['max_over_mean'] or 0:.3f}  n {v['instances']}")
                else:
                    print(f"{label:8s} {tag} {c:34s} {v:.4f}")


if __name__ == "__main__":
    main()
