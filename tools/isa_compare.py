"""Compares the gfx950 device assembly of kernel files between two checkouts (a refactor's proof that the kernels did not move).

    python tools/isa_compare.py --parent-root DIR [--out profiles/rNNx_isa_compare.json] [--parent-listings DIR] [FILE.hip ...]

Compiles every named .hip of eam_rl4co_amd/csrc (default: all of build.SOURCES) in both trees with the flags of
eam_rl4co_amd/build.py plus `--cuda-device-only -S`, and compares per kernel symbol:
  - the instruction stream: the lines between the kernel's label and its end (the kernel descriptor included), comments stripped,
    the __hip_cuid_* symbol and the function index of local labels (.LBB<i>_<n>) ignored;
  - the resources the assembler records: VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy, code length.
Needs hipcc only (no GPU).  Exit status 0 always: the table is the result.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eam_rl4co_amd import build  # noqa: E402

RES = {"vgprs": "NumVgprs", "agprs": "NumAgprs", "sgprs": "TotalNumSgprs", "scratch": "ScratchSize", "lds": "LDSByteSize",
       "occupancy": "Occupancy", "code_bytes": "codeLenInByte"}


def assemble(root: str, src: str, outdir: str, reuse: bool = False) -> str:
    out = os.path.join(outdir, src + ".s")
    if reuse and os.path.exists(out):
        with open(out) as f:
            return f.read()
    cmd = [build.hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", os.path.join(root, "eam_rl4co_amd", "csrc", src), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def kernels(text: str) -> dict:
    """-> {symbol: dict(stream=[...], vgprs=..., ...)} of the .amdhsa kernels of a listing."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    lines = text.split("\n")
    out = {}
    for name in names:
        i = next(n for n, ln in enumerate(lines) if ln.startswith(name + ":")) + 1
        stream = []
        while not lines[i].startswith(".Lfunc_end"):        # the code, then the .amdhsa_kernel descriptor
            ln = lines[i].split(";")[0].strip()
            if ln and "__hip_cuid" not in ln:
                stream.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
            i += 1
        k = {"stream": stream}
        for key, word in RES.items():
            m = None
            for ln in lines[i:i + 60]:
                m = re.match(rf";\s*{word}\s*[:=]\s*(\d+)", ln)
                if m:
                    break
            k[key] = int(m.group(1)) if m else None
        out[name] = k
    return out


def demangle(names):
    try:
        res = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"] + list(names), check=True, capture_output=True, text=True)
        return dict(zip(names, res.stdout.strip().split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def compare(parent_root: str, sources, parent_listings=None) -> dict:
    table = {}
    with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as tt, ThreadPoolExecutor(max_workers=4) as ex:
        if parent_listings:
            os.makedirs(parent_listings, exist_ok=True)
        pa = ex.map(lambda s: kernels(assemble(parent_root, s, parent_listings or tp, reuse=bool(parent_listings))), sources)
        tr = ex.map(lambda s: kernels(assemble(ROOT, s, tt)), sources)
        for src, a, b in zip(sources, pa, tr):
            nice = demangle(sorted(set(a) | set(b)))
            rows = []
            for sym in sorted(set(a) | set(b)):
                ka, kb = a.get(sym), b.get(sym)
                row = {"kernel": nice[sym], "symbol": sym}
                if ka is None or kb is None:
                    row["only_in"] = "tree" if ka is None else "parent"
                else:
                    row["stream_identical"] = ka["stream"] == kb["stream"]
                    row["instructions"] = [len(ka["stream"]), len(kb["stream"])]
                    row["resources_equal"] = all(ka[k] == kb[k] for k in RES if k != "code_bytes")
                    for k in RES:
                        row[k] = ka[k] if ka[k] == kb[k] else [ka[k], kb[k]]
                rows.append(row)
            table[src] = rows
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--out")
    ap.add_argument("--parent-listings", help="keep the parent's listings in this directory and reuse the ones already there")
    ap.add_argument("sources", nargs="*")
    a = ap.parse_args()
    sources = a.sources or build.SOURCES
    table = compare(os.path.abspath(a.parent_root), sources, a.parent_listings)
    rows = [r for rs in table.values() for r in rs]
    differ = [f"{src}: {r['kernel']}" for src, rs in table.items() for r in rs if not r.get("stream_identical", False)]
    res = {"what": "device assembly, parent commit against the tree, per kernel symbol; [parent, tree] where a figure differs",
           "flags": build.FLAGS + ["--cuda-device-only", "-S"], "files": len(table), "kernels": len(rows),
           "stream_identical": sum(bool(r.get("stream_identical")) for r in rows), "stream_differs": differ,
           "resources_differ": [f"{src}: {r['kernel']}" for src, rs in table.items() for r in rs if not r.get("resources_equal", False)],
           "table": table}
    print(json.dumps({k: v for k, v in res.items() if k != "table"}, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
