"""Static instruction counts of one render_pool_kernel instantiation, by opcode class and by section of the loop.

    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S -gline-tables-only \
          -Rpass-analysis=kernel-resource-usage -o tree.s csrc/device/render_pool.hip 2> tree.rpt
    python tools/pool_control_counts.py tree.s [--rpt tree.rpt] [--inst 0,0,128,16] [--src csrc/device/render_pool.hip] [--json out.json --label tree]

Classes are opcode prefixes only (v_ / s_ / ds_ / global_ / other), plus a few named opcodes the control diet is about (s_cselect_b64, v_cndmask_b32,
v_readlane_b32, v_writelane_b32, s_cbranch_*).  Sections come from the .loc line of each instruction (-gline-tables-only adds the lines without changing
the code, and the listing names the chain of call sites an inlined line came from): the innermost line of that chain that lies inside the kernel selects
the section whose anchor comment / lambda precedes it in the source, so a header function inlined into new_ray counts as new_ray.  A static count, good
enough to see where a change landed; the dynamic counts are the SQ counters' (tools/profile_job.sh).
Two parts of the END pass are sections of their own: factor_fetch (from the declaration of the 15 factor registers to the sky lookup) and unwind (from the
path's radiance to the sample store); end_pass is the rest of the pass, and the line "end_pass (all)" sums the three.
With --rpt the compiler's resource report (SGPRs, VGPRs, spills, scratch) of every instantiation is added."""
import argparse
import collections
import json
import os
import re
import sys

NAME = re.compile(r"^(_ZN3crt18render_pool_kernelILi(\d)ELb(\d)ELi(\d+)E(?:Li(\d+)E)?EE\w*):")
ANCHORS = [("new_ray", "auto new_ray ="), ("floor_ray", "auto floor_ray ="), ("world_ray", "auto world_ray ="), ("node_step", "auto node_step ="), ("record_offset", "auto record_offset ="),
           ("load_records", "auto load_records ="), ("tri_step", "auto tri_step ="), ("walk", "for (;;) {"), ("swap_out", "A. swap out"), ("exit_test", "CRT_PACC(0, p0, p1)"),
           ("swap_in", "C. swap in"), ("decide", "B. shading passes"), ("end_pass", "B1. END pass"), ("factor_fetch", "float fk[15];"), ("end_pass", "uint32_t skyTexel = 0u;"),
           ("unwind", "f3 L = miss ?"), ("end_pass", "store_sample(slab, sampleAt, L);"), ("bounce_pass", "B2. BOUNCE pass"), ("epilogue", "CRT_POOL_TIMELINE\n    if (lane == 0 && g_poolTimeline)")]
NAMED = ["s_cselect_b64", "v_cndmask_b32", "v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32", "s_and_saveexec_b64", "s_nop"]


def section_table(src):
    text = open(src).read()
    marks = []
    for name, needle in ANCHORS:
        at = text.find(needle)
        if at >= 0:
            marks.append((text.count("\n", 0, at) + 1, name))
    marks.sort()
    at = text.find("__global__ __launch_bounds__")
    return (text.count("\n", 0, at) + 1 if at >= 0 else 1), marks


def section_of(marks, line):
    sec = "prologue"
    for at, name in marks:
        if line >= at:
            sec = name
    return sec


def kernel_body(path, inst):
    files, body, cur = {}, [], False
    for line in open(path):
        line = line.rstrip("\n")
        f = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', line)
        if f:
            files[int(f.group(1))] = f.group(3) or f.group(2)
        m = NAME.match(line)
        if m:
            cur = (m.group(2), m.group(3), m.group(4), m.group(5) or "16") == inst
            continue
        if cur and line.startswith(".Lfunc_end"):
            break
        if cur:
            body.append(line)
    return files, body


def count(path, inst, src):
    kernel_line, marks = section_table(src)
    _, body = kernel_body(path, inst)
    by_class, by_sec, named = collections.Counter(), collections.defaultdict(collections.Counter), collections.Counter()
    sec, total = "prologue", 0
    for line in body:
        if re.match(r"\s*\.loc\s", line):
            # "; file:line:col @[ file:line:col ] ...": the location and the chain of call sites it was inlined at, innermost first
            for f, n in re.findall(r"([^\s\[]+):(\d+):\d+", line.split(";", 1)[1] if ";" in line else ""):
                if f.endswith("render_pool.hip") and int(n) >= kernel_line:      # (the file's helpers above the kernel count as a header)
                    sec = section_of(marks, int(n))
                    break
            continue
        ins = line.split(";")[0].strip()
        if not ins or ins.startswith(".") or ins.endswith(":"):
            continue
        op = ins.split()[0]
        cls = next((p for p in ("v_", "s_", "ds_", "global_") if op.startswith(p)), "other")
        total += 1
        by_class[cls] += 1
        by_sec[sec][cls] += 1
        if op.startswith("s_cbranch"):
            named["s_cbranch_*"] += 1
            by_sec[sec]["branch"] += 1
        base = re.sub(r"_e(32|64)$", "", op)
        if base in NAMED:
            named[base] += 1
    return {"instructions": total, "by_class": dict(by_class), "named": dict(named),
            "by_section": {k: dict(v, total=sum(n for c, n in v.items() if c != "branch")) for k, v in by_sec.items()}}


def resources(rpt):
    out, cur = {}, None
    for line in open(rpt):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            n = NAME.match(m.group(1) + ":")
            cur = "%s,%s,%s,%s" % (n.group(2), n.group(3), n.group(4), n.group(5) or "16") if n else None
            if cur:
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("listing")
    ap.add_argument("--rpt")
    ap.add_argument("--inst", default="0,0,128,16", help="KIND,COUNT,S,REFBITS")
    ap.add_argument("--src", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cpu-ray-tracer_amd", "csrc", "device", "render_pool.hip"))
    ap.add_argument("--json", help="merge the result into this file under static[<label>]")
    ap.add_argument("--label", default="tree")
    a = ap.parse_args()
    res = count(a.listing, tuple(a.inst.split(",")), a.src)
    res["instantiation"] = a.inst
    if a.rpt:
        res["resources"] = resources(a.rpt)
    if a.json:
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        doc.setdefault("static", {})[a.label] = res
        json.dump(doc, open(a.json, "w"), indent=1, sort_keys=True)
        open(a.json, "a").write("\n")
    print("%s <%s>: %d instructions  %s  %s" % (a.label, a.inst, res["instructions"], res["by_class"], res["named"]))
    for sec, c in sorted(res["by_section"].items(), key=lambda kv: -kv[1]["total"]):
        print("  %-14s %5d  v %4d  s %4d  ds %3d  global %3d  branch %3d" % (sec, c["total"], c.get("v_", 0), c.get("s_", 0), c.get("ds_", 0), c.get("global_", 0), c.get("branch", 0)))
    whole = collections.Counter()
    for sec in ("end_pass", "factor_fetch", "unwind"):
        whole.update(res["by_section"].get(sec, {}))
    print("  %-14s %5d  (end_pass + factor_fetch + unwind)" % ("end_pass (all)", whole["total"]))
    if a.rpt:
        for k, r in sorted(res["resources"].items()):
            print("  <%s> %s" % (k, r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
