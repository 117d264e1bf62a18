"""Timing of ops.moe_bias_grad (csrc/fql_bias.hip) against the torch formulation of the same reduction,
``zeros(E, N).index_add_(0, expert_of_row, g.float())``, in one process: T = 1024 grouped rows, E = 8, N = 4096 and 22016,
float32 and bfloat16 rows, on the even table (128 rows each) and on the skewed table of profiles/r03_skewed_routing.txt
([485, 312, 126, 48, 30, 13, 6, 4]).  The two contenders alternate after warm-up; device events around a window of
``--window`` back-to-back calls (1: a single call, which then carries the launch and event floor of about 10 us).  The rows
are warm in the Infinity Cache for both contenders alike, as they are behind the kernel that produced them.  Prints one JSON
line per case: median and minimum microseconds per call, the bytes the reduction has to read and their rate, and the largest
difference between the two results relative to the float32 bound cnt * 2^-24 * sum |g|."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fused_int4_amd import ops  # noqa: E402

SKEWED = [485, 312, 126, 48, 30, 13, 6, 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--widths", type=int, nargs="+", default=[4096, 22016])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--window", type=int, default=1, help="back-to-back calls between two device events")
    a = ap.parse_args()
    dev = torch.device("cuda")
    T, E = a.rows, a.experts
    tables = {"even": [T // E] * E}
    if T == sum(SKEWED) and E == len(SKEWED):
        tables["skewed"] = SKEWED
    g = torch.Generator(device=dev).manual_seed(0)
    for N in a.widths:
        base = torch.randn(T, N, device=dev, generator=g)
        for dtype in (torch.float32, torch.bfloat16):
            rows = base.to(dtype)
            for name, counts in tables.items():
                cnt = torch.tensor(counts, dtype=torch.int32)
                offs = (torch.cumsum(cnt, 0, dtype=torch.int32) - cnt).to(dev)
                expert_of_row = torch.repeat_interleave(torch.arange(E), cnt.long()).to(dev)
                cnt = cnt.to(dev)
                runs = {"moe_bias_grad": lambda: ops.moe_bias_grad(rows, E, cnt, offs),
                        "torch_index_add": lambda: torch.zeros(E, N, device=dev).index_add_(0, expert_of_row, rows.float())}
                got, ref = runs["moe_bias_grad"](), runs["torch_index_add"]()
                mag = torch.zeros(E, N, device=dev, dtype=torch.float64).index_add_(0, expert_of_row, rows.double().abs())
                bound = cnt.double().reshape(-1, 1) * 2.0 ** -24 * mag
                diff = float(((got.double() - ref.double()).abs() / bound.clamp_min(1e-300)).max())
                times = {k: [] for k in runs}
                for _ in range(a.warmup):
                    for f in runs.values():
                        f()
                torch.cuda.synchronize()
                for _ in range(a.iters):
                    for k, f in runs.items():
                        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        st.record()
                        for _ in range(a.window):
                            f()
                        en.record()
                        en.synchronize()
                        times[k].append(st.elapsed_time(en) * 1e3 / a.window)
                nbytes = T * N * rows.element_size() + E * N * 4
                med = {k: round(statistics.median(v), 1) for k, v in times.items()}
                print(json.dumps({"shape": f"T={T} E={E} N={N} {str(dtype).split('.')[-1]} {name}", "median_us": med,
                                  "min_us": {k: round(min(v), 1) for k, v in times.items()}, "bytes": nbytes,
                                  "moe_bias_grad_TBps": round(nbytes / (med["moe_bias_grad"] * 1e-6) / 1e12, 2),
                                  "speedup_vs_torch": round(med["torch_index_add"] / med["moe_bias_grad"], 2),
                                  "max_diff_over_f32_bound": round(diff, 3)}), flush=True)


if __name__ == "__main__":
    main()
