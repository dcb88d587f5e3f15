#!/usr/bin/env python3
"""Build-time check of the kernel-argument preload of the batch-1 launch chain.

The chain's kernels take what their prologue needs before its first memory instruction as LEADING SCALAR parameters, and the
units that hold them are built with -mllvm -amdgpu-kernarg-preload-count=16 (csrc/Makefile, PRELOAD_UNITS): the command
processor then delivers those kernarg dwords in SGPRs at wave launch.  The compiler decides per kernel how many dwords it
preloads and says so in the kernel descriptor; it stops at the first aggregate parameter and at 14 dwords.  A kernel whose
descriptor promises fewer dwords than its launcher passes as scalars still computes the same, but pays the cold kernarg
miss this was meant to remove -- silently.  This script compiles the units to assembly with the shipped flags, reads
.amdhsa_user_sgpr_kernarg_preload_length per kernel symbol and compares it with the number of scalar dwords of the
kernel's F5E_*_HOT_PARAMS list.  It reads metadata only, no instructions.  usage: check_kernarg_preload.py [csrc dir]"""
import os, re, subprocess, sys, tempfile

csrc = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "f5e-tts_amd", "csrc")
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
mk = open(os.path.join(csrc, "Makefile")).read()
cxxflags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
units = re.search(r"^PRELOAD_UNITS\s*=\s*(.*)$", mk, re.M).group(1).split()
vgpr_form = re.search(r"^(.*):\s*CXXFLAGS \+= -mllvm -amdgpu-mfma-vgpr-form", mk, re.M).group(1)
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]


def hot_dwords(text, family):
    """Scalar dwords of #define F5E_<family>_HOT_PARAMS (a pointer is two), checked against the enum next to it."""
    m = re.search(r"#define F5E_%s_HOT_PARAMS((?:.*\\\n)*.*)\n" % family, text)
    params = [p for p in m.group(1).replace("\\\n", " ").split(",") if p.strip()]
    n = sum(2 if "*" in p else 1 for p in params)
    e = int(re.search(r"F5E_%s_HOT_DWORDS = (\d+)" % family, text).group(1))
    if e != n:
        sys.exit(f"check_kernarg_preload: F5E_{family}_HOT_DWORDS = {e}, but F5E_{family}_HOT_PARAMS lists {n} dwords")
    return n


def src(name):
    return open(os.path.join(csrc, name)).read()


# unit -> [(kernel-name pattern in the mangled symbol, dwords its launcher passes as scalars)]
want = {
    "gemm_bf16": [(r"16gemm_bf16_kernelI", hot_dwords(src("gemm_bf16_args.h"), "GEMM"))],
    "attention": [(r"15attn_fwd_kernelI", hot_dwords(src("attention.hip"), "ATTN")),
                  (r"18attn_fwd_b1_kernelI", hot_dwords(src("attention.hip"), "ATTN"))],
    "conv": [(r"20convpos_split_kernelI", hot_dwords(src("conv.hip"), "CONVPOS"))],
    "gemm_f32": [(r"19gemm_f32_dma_kernelI", hot_dwords(src("gemm_f32.hip"), "GEMM32"))],
    # scalars only; the run ends with the last parameter that fits into 14 dwords whole (rows_per_seq / n)
    "norm": [(r"16adaln_pre_kernelI", 13)],
    "elementwise": [(r"17ode_update_kernelE", 14)],
}
missing = sorted(set(want) - set(units))
if missing:
    sys.exit(f"check_kernarg_preload: {missing} not in PRELOAD_UNITS of the Makefile")

bad = 0
with tempfile.TemporaryDirectory() as td:
    for unit, kernels in want.items():
        out = os.path.join(td, unit + ".s")
        extra = ["-mllvm", "-amdgpu-mfma-vgpr-form"] if f"build/{unit}.o" in vgpr_form.split() else []
        subprocess.check_call([hipcc] + cxxflags + extra + PRELOAD + ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument",
                                                                     os.path.join(csrc, unit + ".hip"), "-o", out])
        sym, got = None, {}
        for ln in open(out):
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
            if m:
                sym = m.group(1)
            m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", ln)
            if m and sym:
                got[sym] = int(m.group(1))
        for pat, n in kernels:
            hits = {s: v for s, v in got.items() if re.search(pat, s)}
            if not hits:
                print(f"FAIL {unit}.hip: no kernel matching {pat} in the assembly")
                bad += 1
            for s, v in sorted(hits.items()):
                if v < n:
                    print(f"FAIL {unit}.hip: {s}: preload length {v} < {n} scalar dwords passed")
                    bad += 1
            if hits:
                print(f"{'ok  ' if all(v >= n for v in hits.values()) else 'FAIL'} {unit}.hip: {len(hits)} x {pat.rstrip('IE')[2:]}: "
                      f"preload length {min(hits.values())} .. {max(hits.values())} (scalar dwords passed: {n})")
sys.exit(1 if bad else 0)
