"""What one evaluation of the linear probe's objective and gradient costs on one MI355X (``python -m uvc_amd.compact_probe fit`` runs a
few hundred per regulariser), against PyTorch.

Arms, at every shape: ``eval`` -- ``ops.probe_eval`` (uvc_probe_eval) at its default ``chunk_rows`` --, ``eval_<rows>`` -- the same at
``chunk_rows`` 16 384, 65 536, 262 144 and n, the sweep that sets the default --, and ``torch`` -- what a user of the library without it
would run: ``F.cross_entropy(X @ W.T + b, y)`` plus ``(l2 / 2) |W|^2`` with autograd, operands in the same type (bf16 X, W and b cast to
bf16 inside the graph).  Shapes (n, D, C): CIFAR-100 features of a DeiT-Small-wide model, and the ImageNet train bank at D = 384 and 768.

Device events, 20 warm-up and 100 timed calls per arm, the arms alternated three times in one process.  The JSON line per shape carries
the ms of every round, the rounds' spread, 4 n D C over the best time as TFLOP/s and as a share of the 2.5 PFLOP/s dense bf16 MFMA peak,
the bytes an evaluation must move at least (X twice) over that time, the largest difference between the arms' gradients relative to the
largest gradient, and eval / torch.  Every shape runs in a child process of its own under a time limit; the first one that fails or runs
out of time ends the run.

    python tools/probe_time.py [cifar in384 in768] [--iters N] [--limit SECONDS] [--precision bf16|fp32]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: n, D, C
SHAPES = {"cifar": (50000, 384, 100), "in384": (1281167, 384, 1000), "in768": (1281167, 768, 1000)}
CHUNKS = (16384, 65536, 262144, None)                # None: n
WARMUP = 20
LIMIT = 900
PEAK_BF16_TFLOPS = 2500.0
L2 = 1e-3


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rounds(arms, iters):
    """{arm: [ms, ms, ms]}: warm-up of every arm, then the arms alternated three times"""
    import torch
    for fn in arms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            ms[k].append(timed(fn, iters))
    return ms


def one(name, iters, precision):
    import torch
    import torch.nn.functional as F
    from uvc_amd import ops
    n, D, Cc = SHAPES[name]
    Cp = -(-Cc // 8) * 8
    op = torch.bfloat16 if precision == "bf16" else torch.float32
    dtype = ops.UVC_BF16 if precision == "bf16" else ops.UVC_F32
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.empty(n, D, device="cuda", dtype=op)
    for j in range(0, n, 1 << 18):                                  # in pieces: no float32 copy of the whole bank
        X[j:j + (1 << 18)] = torch.randn(min(1 << 18, n - j), D, device="cuda", generator=g).to(op)
    y = torch.randint(0, Cc, (n,), device="cuda", generator=g)
    W = torch.zeros(Cp, D, device="cuda")
    W[:Cc] = torch.randn(Cc, D, device="cuda", generator=g) / D ** 0.5
    b = torch.zeros(Cp, device="cuda")
    b[:Cc] = 0.1 * torch.randn(Cc, device="cuda", generator=g)
    default = ops.probe_chunk_rows(n, Cc, dtype)
    outs = dict(dW=torch.empty(Cp, D, device="cuda"), db=torch.empty(Cp, device="cuda"), F=torch.empty(1, dtype=torch.float64, device="cuda"),
                counts=torch.empty(2, dtype=torch.int64, device="cuda"))

    def arm(chunk):
        ws = torch.empty(ops.probe_workspace_bytes(n, D, Cc, dtype, chunk), dtype=torch.uint8, device="cuda")
        return lambda: ops.probe_eval(X, y, W, b, Cc, L2, chunk_rows=chunk, workspace=ws, **outs)
    Wt, bt = W[:Cc].clone().requires_grad_(), b[:Cc].clone().requires_grad_()

    def torch_arm():
        Wt.grad = bt.grad = None
        loss = F.cross_entropy(X @ Wt.to(op).T + bt.to(op), y) + 0.5 * L2 * (Wt * Wt).sum()
        loss.backward()
        return loss
    arms = {"eval": arm(default)}
    for c in CHUNKS:
        rows = n if c is None else c
        if rows <= n and f"eval_{rows}" not in arms:
            arms[f"eval_{rows}"] = arm(rows)
    arms["torch"] = torch_arm
    ms = rounds(arms, iters)
    arms["eval"]()
    torch_arm()
    torch.cuda.synchronize()
    top = float(Wt.grad.abs().max())
    diff = float((outs["dW"][:Cc] - Wt.grad).abs().max()) / top
    best = min(ms["eval"])
    tf = 4.0 * n * D * Cc / (best * 1e-3) / 1e12
    esz = 2 if precision == "bf16" else 4
    spread = {a: round(100 * (max(v) - min(v)) / min(v), 2) for a, v in ms.items()}
    print(json.dumps(dict(shape=name, n=n, D=D, C=Cc, dtype=precision, iters=iters, default_chunk_rows=default,
                          ms={a: [round(t, 4) for t in v] for a, v in ms.items()}, spread_pct=spread, eval_TFLOPs=round(tf, 1),
                          share_of_bf16_peak=round(tf / PEAK_BF16_TFLOPS, 4), X_twice_GBps=round(2.0 * n * D * esz / (best * 1e-3) / 1e9, 1),
                          chunk_bytes=default * Cp * (4 + esz), grad_diff_rel=float(f"{diff:.3e}"),
                          eval_over_torch=round(best / min(ms["torch"]), 4))), flush=True)


def main(argv):
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 100
    precision = argv[argv.index("--precision") + 1] if "--precision" in argv else "bf16"
    if "--one" in argv:
        return one(argv[argv.index("--one") + 1], iters, precision)
    limit = int(argv[argv.index("--limit") + 1]) if "--limit" in argv else LIMIT
    for name in [a for a in argv if a in SHAPES] or list(SHAPES):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--iters", str(iters), "--precision", precision],
                                timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:          # a shape that failed or hung: nothing more is started on the device
            print(json.dumps(dict(shape=name, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
