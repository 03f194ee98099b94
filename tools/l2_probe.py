"""Where does the big-tile GEMM's time go when its activation operand comes from the L2?

    python tools/l2_probe.py [--iters 30] [--out profiles/l2_probe.json]

Times three C2 encoder shapes through the public GEMM entry (irc_gemm_ex), each twice at
equal flops and equal C (and residual) bytes:

  plain    M = 32768 rows of A, as the training step launches it;
  shared   16 batches of M = 2048 whose A stride between batches is 0: every batch reads the
           same 3-12 MB of A, which stays L2-resident, while C, the residual and the tile
           count are the plain launch's.

The two differ only in where A comes from, so their difference is what the activation's L2
misses cost the K loop.  Each is timed with the L2 touch prefetch (irc_gemm_set_l2_touch) on
(mode 2, whatever the launch's width) and off, interleaved, several samples each; the JSON
holds every sample in us per launch.  The ping-pong 256 x 256 kernel is switched off so that
both forms run the big-tile kernel.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "information-retrieval-with-contrastive-learning_amd"))

import torch  # noqa: E402

SHAPES = [  # (name, N, K, epilogue)
    ("ffn1+gelu", 3072, 768, 2),
    ("attn_out+res", 768, 768, 3),
    ("ffn2+res", 768, 3072, 3),
]
M_ALL, BATCH = 32768, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30, help="launches per sample")
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_probe.json"))
    args = ap.parse_args()
    from irc_amd import _lib, ops
    from irc_amd._torch import ptr, stream_ptr

    dev = torch.device("cuda:0")
    m_b = M_ALL // BATCH
    prev_pp = ops.gemm_set_pp(False)
    prev_touch = ops.gemm_set_l2_touch(2)
    result = {"M": M_ALL, "batches": BATCH, "iters": args.iters, "unit": "us per launch",
              "device": torch.cuda.get_device_name(0), "shapes": {}}
    try:
        for name, N, K, epi in SHAPES:
            a = torch.randn((M_ALL, K), device=dev).to(torch.bfloat16)
            b = (torch.randn((N, K), device=dev) * 0.05).to(torch.bfloat16)
            bias = torch.randn((N,), device=dev)
            res = torch.randn((M_ALL, N), device=dev).to(torch.bfloat16) if epi == 3 else None
            out = torch.empty((M_ALL, N), device=dev, dtype=torch.bfloat16)
            st = stream_ptr(dev)

            def launch(shared):
                m, nb = (m_b, BATCH) if shared else (M_ALL, 1)
                _lib.call("irc_gemm_ex", 0, 0, 0, 0, epi, m, N, K, 1.0, ptr(a), K, 0, ptr(b), K,
                          0, ptr(bias), 0, ptr(res), N if res is not None else 0,
                          m * N if res is not None else 0, ptr(out), N, m * N, 0, nb, None, 0,
                          0, st)

            def sample(shared):
                for _ in range(3):
                    launch(shared)
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    launch(shared)
                e1.record()
                torch.cuda.synchronize()
                return round(e0.elapsed_time(e1) * 1e3 / args.iters, 2)

            rows = {f"{form}_touch_{t}": [] for form in ("plain", "shared") for t in ("on", "off")}
            for _ in range(args.samples):
                for touch in (True, False):
                    ops.gemm_set_l2_touch(2 if touch else 0)  # 2: every launch that can
                    for shared in (False, True):
                        key = f"{'shared' if shared else 'plain'}_touch_{'on' if touch else 'off'}"
                        rows[key].append(sample(shared))
            rows.update(N=N, K=K, epilogue=epi, a_mbytes_plain=round(M_ALL * K * 2 / 1e6, 1),
                        a_mbytes_shared=round(m_b * K * 2 / 1e6, 1))
            result["shapes"][name] = rows
            print(name, json.dumps(rows), flush=True)
    finally:
        ops.gemm_set_l2_touch(prev_touch)
        ops.gemm_set_pp(prev_pp)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
