#!/usr/bin/env python3
"""Turns a kernel trace of the Thomas solves into the rows of tests/golden/ipk_plans.json.

Input, per case NAME of a run directory (one process per case, rocprofv3 --kernel-trace -f csv):
  DIR/NAME/**/*kernel_trace.csv   the trace: every dispatch with kernel name, grid, workgroup, LDS
                                  (LDS_Block_Size of rocprofv3 1.x on ROCm 7 is the STATIC LDS of the
                                  kernel: the dynamic size of a launch is not in it -- `lds_static`)
  DIR/NAME.err                    stderr of a development build that prints, per ipk_launch call,
      IPKSOLVE elem=E axis=A m=M0,M1,M2 nbatch=N bstride=B add=S need=K   (the solve as it is seen;
                                   need: the warm-up length of the hierarchy's Thomas tables)
      IPKARGS fam=F W= n_glob= K= KR= P= S= nchunk=                        (the launch arguments)
  (nothing that prints per launch is committed; tools/ipk_trace.md has the lines to add, where they go,
   and the run that produces DIR: tools/ipk_trace_case.py, one process per case).
A trace does not show kernel arguments and does not say which solve a dispatch belongs to: the log
gives the solves in order, the trace the dispatches in order, and the two are walked together --
each solve takes the next dispatch(es) of its family's kernels, and a name that does not fit stops
the conversion. Dispatches of k_ipk* kernels that ipk_launch does not launch (k_ipk_plane_fc, the
N-D kernels) are passed over.

  tools/ipk_trace_to_plans.py rows DIR [--env NAME=switch=value,...] > tests/golden/ipk_plans.json
  tools/ipk_trace_to_plans.py dispatches DIR    every k_ipk* dispatch of every case, one per line
                                                (to diff two builds: name, grid, workgroup, LDS)
"""
import csv
import glob
import json
import os
import re
import sys

FAMILY_KERNELS = {
    "Spec": ["k_ipk_spec_fwd", "k_ipk_spec_check", "k_ipk_spec_fix", "k_ipk_spec_bwd", "k_ipk_spec_check",
             "k_ipk_spec_fix"],
    "LdsContigChunked": ["k_ipk_lds_contig"], "Dma": ["k_ipk_dma"], "Stream": ["k_ipk_stream"],
    "LdsContig": ["k_ipk_lds_contig"], "LdsStrided": ["k_ipk_lds_strided"], "Thread": ["k_ipk"],
}
OURS = {k for v in FAMILY_KERNELS.values() for k in v} | {"k_ipk_spec_apply"}


def short_name(full):
    """'void mgh::k_ipk_dma<float, 16, 10, 1, true>(unsigned int, ...)' -> 'k_ipk_dma<float, 16, 10, 1, true>'"""
    s = re.sub(r"^void\s+", "", full.strip())
    depth, end = 0, len(s)
    for i, ch in enumerate(s):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            end = i
            break
    s = s[:end].strip()
    s = re.sub(r"\(anonymous namespace\)::", "", s)
    return re.sub(r"^(\w+::)+", "", s).replace(".kd", "")


def base_name(short):
    return short.split("<")[0]


def read_trace(case_dir):
    files = sorted(glob.glob(os.path.join(case_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no kernel trace under " + case_dir)
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f, newline="")))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    out = []
    for r in rows:
        name = short_name(r["Kernel_Name"])
        if not name.startswith("k_ipk"):
            continue
        wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
        grid = [int(r["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg)]  # work-items -> workgroups
        out.append({"kernel": name, "grid": grid[0] * grid[1] * grid[2], "workgroup": wg[0] * wg[1] * wg[2],
                    "lds_static": int(r["LDS_Block_Size"])})
    return out


def read_log(path):
    solves = []
    for line in open(path, errors="replace"):
        if line.startswith("IPKSOLVE "):
            kv = dict(t.split("=") for t in line.split()[1:])
            solves.append({"elem": int(kv["elem"]), "axis": int(kv["axis"]), "m": [int(x) for x in kv["m"].split(",")],
                           "nbatch": int(kv["nbatch"]), "batch_stride": int(kv["bstride"]), "add": int(kv["add"]),
                           "chunk_need": int(kv["need"])})
        elif line.startswith("IPKARGS "):
            kv = dict(t.split("=") for t in line.split()[1:])
            solves[-1]["family"] = kv.pop("fam")
            solves[-1]["args"] = {k: int(v) for k, v in kv.items()}
    return solves


def case_rows(run_dir, case):
    trace = [d for d in read_trace(os.path.join(run_dir, case)) if base_name(d["kernel"]) in OURS]
    solves = read_log(os.path.join(run_dir, case + ".err"))
    rows, pos, i = [], 0, 0
    while i < len(solves):
        s = solves[i]
        i += 1
        calls = [s]
        if s["family"] == "ThreadBatches":  # one call per box follows, each with its own lines
            calls = solves[i:i + s["nbatch"]]
            i += s["nbatch"]
            s["family"] = "Thread"
        s["dispatches"] = []
        for c in calls:
            want = list(FAMILY_KERNELS[c["family"]]) + (["k_ipk_spec_apply"] if c["family"] == "Spec" and c["add"] else [])
            got = trace[pos:pos + len(want)]
            pos += len(want)
            if [base_name(d["kernel"]) for d in got] != want:
                raise SystemExit("%s: solve %r expected %r, the trace has %r" % (case, c, want, got))
            s["dispatches"] += got
        rows.append(s)
    if pos != len(trace):
        raise SystemExit("%s: %d dispatches of the trace belong to no solve of the log" % (case, len(trace) - pos))
    return rows


def cases_of(run_dir):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(run_dir, "*.err")))


def main():
    mode, run_dir = sys.argv[1], sys.argv[2]
    if mode == "dispatches":
        for case in cases_of(run_dir):
            for d in read_trace(os.path.join(run_dir, case)):
                print("%s\t%s\t%d\t%d\t%d" % (case, d["kernel"], d["grid"], d["workgroup"], d["lds_static"]))
        return
    env = {}
    for a in sys.argv[3:]:
        if a.startswith("--env="):
            name, rest = a[6:].split("=", 1)
            env[name] = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in rest.split(","))
    out, seen = [], {}
    for case in cases_of(run_dir):
        for r in case_rows(run_dir, case):
            tuning = dict(env.get(case, {}), chunk_need=r["chunk_need"])
            key = json.dumps([r["elem"], r["axis"], r["m"], r["nbatch"], r["batch_stride"], r["add"], tuning], sort_keys=True)
            row = {"from": [case], "elem": r["elem"], "axis": r["axis"], "m": r["m"], "nbatch": r["nbatch"],
                   "batch_stride": r["batch_stride"], "add": r["add"], "tuning": tuning, "family": r["family"],
                   "args": r["args"], "dispatches": r["dispatches"]}
            if key in seen:
                old = seen[key]
                if (old["family"], old["args"], old["dispatches"]) != (row["family"], row["args"], row["dispatches"]):
                    raise SystemExit("the same solve was planned in two ways: %r / %r" % (old, row))
                if case not in old["from"]:
                    old["from"].append(case)
                continue
            seen[key] = row
            out.append(row)
    print("[")
    print(",\n".join(" " + json.dumps(r) for r in out))
    print("]")


if __name__ == "__main__":
    main()
