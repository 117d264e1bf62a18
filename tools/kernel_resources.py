#!/usr/bin/env python3
"""Print per-kernel register / LDS / spill figures from the gfx950 assembly metadata
(`make -C <pkg>/csrc asm` writes fql_int4.gfx950.s, `asm-lora` writes fql_lora.gfx950.s).
With --require-no-scratch only offending kernels and a count are printed, and the exit status is 1 if any kernel spills or has a private segment (the adapter kernels of
fql_lora.h, gated variants and swiglu_bwd included, must not)."""
import re
import sys

strict = "--require-no-scratch" in sys.argv
args = [x for x in sys.argv[1:] if not x.startswith("--")]
path = args[0] if args else "fused-4-bit-dequantize-linear-cuda-kernel_amd/csrc/fql_int4.gfx950.s"
txt = open(path).read()
kernels, bad = 0, []
meta = txt[txt.index("amdhsa.kernels:"):]
for blk in re.split(r"\n  - ", meta)[1:]:
    g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
    name = g("name")
    line = (f"{name[:70]:70s} vgpr={g('vgpr_count'):>4s} agpr={g('agpr_count'):>3s} sgpr={g('sgpr_count'):>3s} "
          f"lds={g('group_segment_fixed_size'):>6s} spill={g('vgpr_spill_count')} scratch={g('private_segment_fixed_size')}")
    if not strict:
        print(line)
    if name != "?":
        kernels += 1
        if g("vgpr_spill_count") != "0" or g("private_segment_fixed_size") != "0":
            bad.append(name)
            print(line)
if strict:
    print(f"{kernels} kernels, {len(bad)} with spills or scratch")
    sys.exit(1 if bad else 0)
