#!/usr/bin/env python3
"""Vector / scalar / memory instructions per loop of the scan kernels, counted from the ISA of THIS tree
(lsqrrecipes_amd/csrc/lsqr_hip.s: `make -C lsqrrecipes_amd/csrc asm`), so that the `useful` instruction counts bench.py
prices the issue roof with (SCAN_USEFUL, counted from the source) can be read next to what the compiler emitted
(VERDICT r04 item 4).  Runs on the CPU (hipcc cross-compiles); writes profiles/r05_isa_counts.json, stamped with the
kernel source hash bench.py checks.

    python tools/isa_counts.py [out.json]"""
import collections
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import kernel_source_hash  # noqa: E402

CSRC = os.path.join(ROOT, "lsqrrecipes_amd", "csrc")
# (key, kernel, its template arguments as c++filt prints them): every key selects exactly one instantiation.  The forms
# of the counted scan are written by name (cells.h: PairsForm, BoundsForm); PP = cell size / 128, then BS and LDSB.
PLANE = "lsqr::PlaneCell<3>"
# A trailing "float const*" selects the instantiation that opens a cell from the index's fp32 tiles (scan_tiles=1); the
# key without it is the same form on cells_load (scan_tiles=0).  "cell_open" of a k_scan_pairs key counts the cell
# loop's own instructions (share arithmetic + cell open, the loops inside it left out): the difference between a key
# and its _tiles twin is what opening a cell from the sorted copy costs.
TILES = "float const*"
KERNELS = [("k_scan_pairs_plane", "k_scan_pairs", [PLANE, "4", "256", "true", "PairsForm::PackedRecheck"]),  # scan_tiles=0
           ("k_scan_pairs_plane_tiles", "k_scan_pairs", [PLANE, "4", "256", "true", "PairsForm::PackedRecheck", TILES]),  # what runs
           ("k_scan_pairs_sphere_tiles", "k_scan_pairs", ["lsqr::SphereCell<3>", "4", "256", "true", "PairsForm::General", TILES]),
           ("k_scan_pairs_line_tiles", "k_scan_pairs", ["lsqr::LineCell<3>", "2", "256", "true", "PairsForm::General", TILES]),
           ("k_scan_pairs_plane_whole_cell", "k_scan_pairs", [PLANE, "4", "256", "true", "PairsForm::Packed"]),  # scan_recheck=0
           ("k_scan_pairs_plane_groups", "k_scan_pairs", [PLANE, "4", "256", "true", "PairsForm::Lean"]),  # scan_pack=0
           ("k_scan_pairs_plane_general", "k_scan_pairs", [PLANE, "4", "256", "true", "PairsForm::Prepared"]),  # scan_lean=0
           ("k_scan_pairs_plane_unprepared", "k_scan_pairs", [PLANE, "4", "256", "true", "PairsForm::General"]),  # scan_prepared=0 scan_lean=0
           ("k_cells_bounds_plane", "k_cells_bounds", [PLANE, "4", "BoundsForm::PreparedMask"]),  # mask-only counting pass: what runs
           ("k_cells_bounds_plane_count", "k_cells_bounds", [PLANE, "4", "BoundsForm::PreparedCount"]),  # scan_pack=0: count-only
           ("k_cells_bounds_plane_general", "k_cells_bounds", [PLANE, "4", "BoundsForm::Prepared"]),  # scan_lean=0
           ("k_scan_pairs_sphere", "k_scan_pairs", ["lsqr::SphereCell<3>", "4", "256", "true", "PairsForm::General"]),
           ("k_scan_pairs_line", "k_scan_pairs", ["lsqr::LineCell<3>", "2", "256", "true", "PairsForm::General"]),
           ("k_scan_us_f32", "k_scan_us_f32", ["lsqr::USModel<true>", "2"]),
           ("k_scan_dense_h16", "k_scan_dense_h16", ["64", "false", "0"]),
           ("k_scan_us_h16", "k_scan_us_h16", ["true"]),
           ("k_scan_phantom_h16", "k_scan_phantom_h16", None),
           ("k_lm_persist_us", "k_lm_persist", ["lsqr::USModel<true>", "0"])]


def enum_values(name):
    """enumerators of `enum class <name>` in cells.h, in order: c++filt prints a form as (lsqr::<name>)<index>"""
    m = re.search(r"enum class %s \{([^}]*)\}" % name, open(os.path.join(CSRC, "cells.h")).read())
    return [e.strip() for e in m.group(1).split(",")]


def template_args(demangled):
    """(kernel, [top-level template arguments]) of `[void ]lsqr::kernel[<args>](parameters)`, or None"""
    m = re.match(r"(?:void )?lsqr::(\w+)", demangled)
    if not m:
        return None
    rest = demangled[m.end():]
    if not rest.startswith("<"):
        return (m.group(1), None) if rest.startswith("(") else None
    args, depth, cur = [], 0, ""
    for ch in rest:
        if ch in "<(":
            depth += 1
            if depth == 1:
                continue
        elif ch in ">)":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return m.group(1), args
        if ch == "," and depth == 1:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return None


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_pk_"):
        return "valu_packed"
    if op.startswith("v_cmp"):
        return "valu_cmp"
    if op.startswith("v_"):
        return "valu_other"
    if op.startswith("s_waitcnt") or op.startswith("s_nop") or op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "control"
    if op.startswith("s_load") or op.startswith("s_buffer"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r05_isa_counts.json")
    asm = os.path.join(CSRC, "lsqr_hip.s")
    if not os.path.exists(asm) or os.path.getmtime(asm) < max(
            os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))):
        subprocess.check_call(["make", "-C", CSRC, "asm"])
    text = open(asm).read()
    # function bodies: "<mangled>:" ... ".Lfunc_end"
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(_Z[\w]+):\s*(?:;.*)?$", text, re.M)]
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        sys.exit("neither c++filt nor llvm-cxxfilt on PATH: kernels are selected by their demangled names")
    # (binutils' c++filt does not know _Float16, "DF16_": written as half, "Dh", neither of them a substitution candidate,
    # the name demangles; only the parameter list reads differently)
    names = subprocess.run([filt], input="\n".join(n.replace("DF16_", "Dh") for _, n in starts), capture_output=True,
                           text=True, check=True).stdout.split("\n")
    parsed = [(p, n, template_args(d)) for (p, n), d in zip(starts, names)]
    forms = {"%s::%s" % (e, v): "(lsqr::%s)%d" % (e, i)
             for e in ("PairsForm", "BoundsForm") for i, v in enumerate(enum_values(e))}
    res = {}
    bad = []
    for key, kernel, args in KERNELS:
        want = None if args is None else [forms.get(a, a) for a in args]
        cand = [(p, n) for p, n, t in parsed if t == (kernel, want)]
        if len(cand) != 1:
            bad.append("%s: %d instantiations of %s<%s>" % (key, len(cand), kernel, ", ".join(args or [])))
            continue
        best = (cand[0][0], cand[0][1], text.index(".Lfunc_end", cand[0][0]))
        body = text[best[0]:best[2]].split("\n")
        loops = collections.OrderedDict()
        cur = ("entry", 0)
        for li, line in enumerate(body):
            m = re.match(r"^(\.LBB\d+_\d+):\s*;?\s*(.*)$", line)
            if m:
                lab, rest = m.group(1), m.group(2)
                # a nested loop's header carries its parents on the label line and "This (Inner) Loop Header: Depth=n"
                # on one of the comment lines that follow
                k = li + 1
                while "Parent Loop" in rest and k < len(body) and body[k].lstrip().startswith(";"):
                    if "Loop Header" in body[k]:
                        rest = body[k]
                        break
                    k += 1
                d = re.search(r"Depth=(\d+)", rest)
                h = re.search(r"Header=(BB\d+_\d+)", rest)
                if "Loop Header" in rest and d:
                    cur = (lab.lstrip("."), int(d.group(1)))
                elif h and d:
                    cur = (h.group(1), int(d.group(1)))
                else:
                    cur = ("straight", 0)
                continue
            if not line.startswith("\t") or line.startswith("\t.") or line.startswith("\t;"):
                continue
            op = line.split()[0]
            loops.setdefault(cur, collections.Counter())[classify(op)] += 1
            loops[cur]["op:" + op] += 1
        rows = []
        for (hdr, depth), cnt in loops.items():
            if depth == 0:
                continue
            valu = cnt["valu_packed"] + cnt["valu_cmp"] + cnt["valu_other"]
            top = {k[3:]: v for k, v in cnt.items() if k.startswith("op:") and k.startswith("op:v_")}
            rows.append({"loop": hdr, "depth": depth, "valu": valu, "valu_packed": cnt["valu_packed"],
                         "valu_cmp": cnt["valu_cmp"], "mfma": cnt["mfma"], "salu": cnt["salu"], "smem": cnt["smem"],
                         "lds": cnt["lds"], "vmem": cnt["vmem"], "control": cnt["control"],
                         "vector_ops": dict(sorted(top.items(), key=lambda kv: -kv[1])[:14])})
        # the cell loop of k_scan_pairs: the outermost loop with the most instructions of its own
        cell_open = None
        if kernel == "k_scan_pairs":
            (hdr, _), cnt = max(((k, c) for k, c in loops.items() if k[1] == 1),
                                key=lambda kc: sum(v for o, v in kc[1].items() if o.startswith("op:")))
            cell_open = {"loop": hdr, "valu": cnt["valu_packed"] + cnt["valu_cmp"] + cnt["valu_other"],
                         "vmem": cnt["vmem"], "salu": cnt["salu"], "v_cvt_f32_f64": cnt["op:v_cvt_f32_f64_e32"],
                         "v_add_f64": cnt["op:v_add_f64"]}
        rows.sort(key=lambda r: (-r["depth"], -r["valu"]))
        # the loop with the most packed instructions = the packed fp32 filter's body (level 2 of the point models)
        l2 = max(rows, key=lambda r: r["valu_packed"]) if rows else None
        res[key] = {"function": best[1][:120], "loops": rows, "cell_open": cell_open,
                    # counting pass: the loop with the most vector instructions (its header block "LBBn_m" and the
                    # blocks "BBn_m" inside it taken together) is the four-cells-at-a-time loop
                    "valu_per_cell": max(sum(r["valu"] for r in rows if r["loop"].lstrip("L") == n)
                                         for n in {r["loop"].lstrip("L") for r in rows}) / 4.0
                    if key.startswith("k_cells_bounds") and rows else None,
                    "packed_body": {"loop": l2["loop"], "valu": l2["valu"], "valu_packed": l2["valu_packed"],
                                    "valu_cmp": l2["valu_cmp"], "salu": l2["salu"]} if l2 else None}
    if bad:  # (nothing is written: a profile with some of its keys would pass for a whole one)
        sys.exit("no single kernel for\n  " + "\n  ".join(bad))
    out = {"what": "tools/isa_counts.py: instructions per loop of the scan kernels in this tree's ISA (one pass over a loop "
                   "body; a body the compiler unrolled covers several source iterations)",
           "kernel_source_hash": kernel_source_hash(), "kernels": res}
    json.dump(out, open(out_path, "w"), indent=1)
    for k, v in res.items():
        print(k, v["packed_body"] if v["valu_per_cell"] is None else {"valu_per_cell": v["valu_per_cell"]})


if __name__ == "__main__":
    main()
