#!/usr/bin/env python3
"""usage: tools/kernel_listing.py [LIB] [--against OTHER] [--sizes]

The gfx950 kernels inside a built libhssfsst.so (default: the tree's own), one entry per kernel symbol: its ``llvm-objdump -d``
listing -- instruction text and encoding, the address column dropped, ended at the symbol's size -- and its ``llvm-readelf
--notes`` entry (arguments, VGPRs, AGPRs, SGPRs, LDS, scratch).  Prints the number of kernels and of instructions and one sha256
over (symbol, instructions); every code object of the library is read (_lib._unbundle), and a symbol that two of them define is
an error.  --against OTHER: the same for a second library, then which symbols only one of them has, whose listings differ (as a
unified diff) and whose notes differ; exit status 1 when anything does.  --sizes: code bytes per kernel, largest first.
Hashes and diffs what two builds made of the same source, e.g. before and after code moved between translation units."""
import argparse
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from heart_sounds_segmentation_amd import _lib  # noqa: E402


def kernels(path: str) -> dict:
    """{kernel symbol: {"code": [instruction lines], "bytes": size, "notes": text of its metadata entry, "unit": code object index}}"""
    tools = _lib._llvm_tools("clang-offload-bundler", "llvm-objdump", "llvm-readelf")

    def run(*cmd):
        return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout

    out = {}
    with tempfile.TemporaryDirectory() as td:
        for unit, obj in enumerate(_lib._unbundle(tools, path, td)):
            notes = {}
            for blk in re.split(r"\n\s*- \.agpr_count:", run(tools["llvm-readelf"], "--notes", obj))[1:]:
                blk = ".agpr_count:" + re.split(r"\namdhsa\.|\n\.\.\.", blk)[0]
                notes[re.search(r"\.name:\s+(\S+)", blk).group(1)] = "\n".join(ln.strip() for ln in blk.split("\n") if ln.strip())
            extent = {}                                   # symbol -> (address, size) of every function with code
            for ln in run(tools["llvm-readelf"], "-s", "-W", obj).split("\n"):
                f = ln.split()
                if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
                    extent[f[7]] = (int(f[1], 16), int(f[2]))
            if set(extent) != set(notes):
                raise RuntimeError(f"{path}: code object {unit}: functions {sorted(set(extent) ^ set(notes))[:3]} ... are not kernels with metadata")
            name = None
            for ln in run(tools["llvm-objdump"], "-d", "--mcpu=gfx950", obj).split("\n"):
                head = re.match(r"^[0-9a-f]+ <(\S+)>:$", ln)
                if head:
                    name = head.group(1) if head.group(1) in extent else None
                    if name in out:
                        raise RuntimeError(f"{path}: {name} is defined in code objects {out[name]['unit']} and {unit}")
                    if name:
                        out[name] = {"code": [], "bytes": extent[name][1], "notes": notes[name], "unit": unit}
                    continue
                ins = re.match(r"^\s+(\S.*?)\s*// ([0-9A-F]+): (.*)$", ln)
                if name and ins and int(ins.group(2), 16) < extent[name][0] + extent[name][1]:
                    out[name]["code"].append(f"{ins.group(1)} // {ins.group(3)}")
    return out


def digest(ks: dict) -> str:
    h = hashlib.sha256()
    for name in sorted(ks):
        h.update((name + "\n" + "\n".join(ks[name]["code"]) + "\n").encode())
    return h.hexdigest()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib", nargs="?", default=_lib.LIB_PATH)
    ap.add_argument("--against")
    ap.add_argument("--sizes", action="store_true")
    a = ap.parse_args()
    mine = kernels(a.lib)
    print(f"{a.lib}: {len(mine)} kernels in {len({k['unit'] for k in mine.values()})} code objects, "
          f"{sum(len(k['code']) for k in mine.values())} instructions, sha256 {digest(mine)}")
    if a.sizes:
        for name in sorted(mine, key=lambda n: -mine[n]["bytes"]):
            print(f"  {mine[name]['bytes']:9d} B  code object {mine[name]['unit']}  {name}")
    if not a.against:
        return 0
    other = kernels(a.against)
    print(f"{a.against}: {len(other)} kernels in {len({k['unit'] for k in other.values()})} code objects, "
          f"{sum(len(k['code']) for k in other.values())} instructions, sha256 {digest(other)}")
    bad = 0
    for name in sorted(set(mine) ^ set(other)):
        print(f"only in {a.lib if name in mine else a.against}: {name}")
        bad += 1
    both = sorted(set(mine) & set(other))
    for name in both:
        if mine[name]["code"] != other[name]["code"]:
            bad += 1
            print(f"listing differs: {name}")
            sys.stdout.writelines(ln + "\n" for ln in difflib.unified_diff(other[name]["code"], mine[name]["code"], a.against, a.lib, n=2, lineterm=""))
        if mine[name]["notes"] != other[name]["notes"]:
            bad += 1
            print(f"notes differ: {name}")
            sys.stdout.writelines(ln + "\n" for ln in difflib.unified_diff(other[name]["notes"].split("\n"), mine[name]["notes"].split("\n"),
                                                                             a.against, a.lib, n=0, lineterm=""))
    print(f"{len(both)} kernels in both; {len(both) - sum(1 for n in both if mine[n]['code'] != other[n]['code'])} equal listings, "
          f"{len(both) - sum(1 for n in both if mine[n]['notes'] != other[n]['notes'])} equal notes")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
