#!/usr/bin/env python3
"""Digest of every kernel's gfx950 code: two trees compile a kernel to the same instructions, registers and kernel descriptor
iff they print the same line for it (CPU only: hipcc -S --cuda-device-only, no GPU).

    python3 tools/kernel_asm_digests.py [--probes] [--tree DIR] [--keep DIR] [FILE.hip ...] > new.txt
    python3 tools/kernel_asm_digests.py [--probes] --tree /path/to/parent/checkout > parent.txt && diff parent.txt new.txt

One line per kernel, `file  kernel-symbol  digest`, sorted: the first 16 hex digits of the SHA-256 over the listing's text from the
kernel's label through its `.end_amdhsa_kernel`.  A whole-file comparison does not work for a change that only reorders the
instantiations of a file: the basic-block labels carry the function's ordinal in the file (`.LBB0_4` becomes `.LBB6_4`), so
`BB<n>_` is read as `BB_`, and the blanks that pad a block label's comment to its column (one less when the ordinal grows a digit)
as one.  Nothing else is normalised: any other difference is a difference.

Files: every csrc/*.hip by default, built with the Makefile's flags (check_inline_asm.PER_FILE_FLAGS mirrors its FLAGS_*);
--probes adds -DVIT_PROBES and the probe-only kernels under tools/probes/ (the Makefile's PROBE_ONLY_SRC).
"""
from __future__ import annotations

import argparse, concurrent.futures, glob, hashlib, os, re, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_inline_asm as lint  # noqa: E402

PROBE_ONLY = ["vit_gemm_bf16_w4.hip"]  # under tools/probes/


def kernel_texts(text: str):
    """[(symbol, text)] for every kernel of an AMDGPU listing: from its label through its `.end_amdhsa_kernel`."""
    out, name, start = [], None, 0
    lines = text.split("\n")
    for n, raw in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", raw)
        if m and not m.group(1).startswith(".L"):
            name, start = m.group(1), n
        elif name is not None and raw.strip() == ".end_amdhsa_kernel":
            out.append((name, "\n".join(lines[start:n + 1])))
            name = None
    return out


def digest(kernel_text: str) -> str:
    text = re.sub(r"BB\d+_", "BB_", kernel_text)
    # a block label's comment (`; =>This Inner Loop Header`) is padded to a fixed column: one blank less when the ordinal grows a digit
    text = re.sub(r"^(\.LBB_\d+:) +;", r"\1 ;", text, flags=re.M)
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*", help="HIP sources (default: every csrc/*.hip of the tree)")
    ap.add_argument("--tree", default=lint.ROOT, help="checkout to compile (default: this one)")
    ap.add_argument("--probes", action="store_true", help="the probe build: -DVIT_PROBES, and the kernels of tools/probes/")
    ap.add_argument("--keep", help="directory to keep the generated .s files in")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--asm", nargs="+", default=[], metavar="FILE.s", help="digest these assembly listings as they are instead of compiling")
    a = ap.parse_args()
    if a.asm:
        for row in sorted((os.path.basename(p)[:-2] + ".hip", name, digest(body)) for p in a.asm for name, body in kernel_texts(open(p).read())):
            print("  ".join(row))
        return 0
    csrc = os.path.join(a.tree, "vision-transformer-opencl_amd", "csrc")
    srcs = a.files or sorted(glob.glob(os.path.join(csrc, "*.hip")))
    if a.probes and not a.files:
        srcs += [os.path.join(a.tree, "tools", "probes", f) for f in PROBE_ONLY]
    extra = ["-fPIC", "-I" + csrc] + (["-DVIT_PROBES"] if a.probes else [])
    with tempfile.TemporaryDirectory() as td:
        outdir = a.keep or td
        os.makedirs(outdir, exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(a.jobs, len(srcs)))) as ex:
            listings = list(ex.map(lambda s: lint.compile_to_asm(s, outdir, extra, root=a.tree), srcs))
        rows = []
        for src, path in zip(srcs, listings):
            rows += [(os.path.basename(src), name, digest(body)) for name, body in kernel_texts(open(path).read())]
    for row in sorted(rows):
        print("  ".join(row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
