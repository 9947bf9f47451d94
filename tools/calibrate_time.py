"""What one evaluation of the calibration objective and its gradient costs on one MI355X (``python -m uvc_amd.compact_calibrate fit`` runs a
few to a few hundred), against PyTorch.

Arms, at every shape: ``eval_temperature`` and ``eval_vector`` -- ``ops.calib_eval`` (uvc_calib_eval) with one scale, and with a scale and a
shift per class -- and ``torch_temperature`` / ``torch_vector`` -- what a user of the library without it would run: autograd through
``F.cross_entropy(logits * a + d, y)``.  The logits are float32 (a bank's type; bf16 plays no part).  Shapes (n, C): a CIFAR-100 test
split, the ImageNet validation set and the ImageNet train set; the row stride is C rounded up to 8, a compact file's head width.

Device events, 20 warm-up and 100 timed calls per arm, the arms alternated three times in one process.  The JSON line per shape carries the
ms of every round, the rounds' spread, n ld 4 bytes over the kernel's best time in GB/s (to be read against the ``read`` rows of
profiles/r1_bw_probe_hbm_ceilings.csv; only a shape whose logits pass the 256 MiB Infinity Cache is an HBM figure), the largest difference
between the arms' gradients relative to the largest gradient, and eval / torch per mode.  Every shape runs in a child process of its own
under a time limit; the first one that fails or runs out of time ends the run.

    python tools/calibrate_time.py [cifar inval intrain] [--iters N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: n, C
SHAPES = {"cifar": (10000, 100), "inval": (50000, 1000), "intrain": (1281167, 1000)}
WARMUP = 20
LIMIT = 900


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


def one(name, iters):
    import torch
    import torch.nn.functional as F
    from uvc_amd import ops
    n, Cc = SHAPES[name]
    ld = -(-Cc // 8) * 8
    g = torch.Generator(device="cuda").manual_seed(0)
    Z = torch.empty(n, ld, device="cuda")
    for j in range(0, n, 1 << 18):
        Z[j:j + (1 << 18)] = 3.0 * torch.randn(min(1 << 18, n - j), ld, device="cuda", generator=g)
    y = torch.randint(0, Cc, (n,), device="cuda", generator=g)
    s = torch.full((1,), 0.8, device="cuda")
    a = 0.5 + torch.rand(Cc, device="cuda", generator=g)
    d = 0.5 * torch.randn(Cc, device="cuda", generator=g)
    ws = torch.empty(ops.calib_workspace_bytes(n, ld, Cc), dtype=torch.uint8, device="cuda")
    outs = dict(F=torch.empty(1, dtype=torch.float64, device="cuda"), counts=torch.empty(2, dtype=torch.int64, device="cuda"), workspace=ws)
    ds1, dsv, ddv = torch.empty(1, device="cuda"), torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
    st, at, dt = s.clone().requires_grad_(), a.clone().requires_grad_(), d.clone().requires_grad_()
    Zv = Z[:, :Cc]

    def torch_temperature():
        st.grad = None
        loss = F.cross_entropy(Zv * st, y)
        loss.backward()
        return loss

    def torch_vector():
        at.grad = dt.grad = None
        loss = F.cross_entropy(Zv * at + dt, y)
        loss.backward()
        return loss
    arms = {"eval_temperature": lambda: ops.calib_eval(Z, y, s, None, Cc, dscale=ds1, **outs),
            "eval_vector": lambda: ops.calib_eval(Z, y, a, d, Cc, dscale=dsv, dshift=ddv, **outs),
            "torch_temperature": torch_temperature, "torch_vector": torch_vector}
    ms = rounds(arms, iters)
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    diff = max(float((ds1 - st.grad).abs().max() / st.grad.abs().max()), float((dsv - at.grad).abs().max() / at.grad.abs().max()),
               float((ddv - dt.grad).abs().max() / dt.grad.abs().max()))
    spread = {k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()}
    gbps = {m: round(n * ld * 4 / (min(ms["eval_" + m]) * 1e-3) / 1e9, 1) for m in ("temperature", "vector")}
    print(json.dumps(dict(shape=name, n=n, C=Cc, ld=ld, iters=iters, blocks=ops.calib_blocks(n, ld), logits_MB=round(n * ld * 4 / 1e6, 1),
                          ms={k: [round(t, 4) for t in v] for k, v in ms.items()}, spread_pct=spread, logits_GBps=gbps,
                          grad_diff_rel=float(f"{diff:.3e}"),
                          eval_over_torch={m: round(min(ms["eval_" + m]) / min(ms["torch_" + m]), 4) for m in ("temperature", "vector")})), flush=True)


def main(argv):
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 100
    if "--one" in argv:
        return one(argv[argv.index("--one") + 1], iters)
    limit = int(argv[argv.index("--limit") + 1]) if "--limit" in argv else LIMIT
    for name in [a for a in argv if a in SHAPES] or list(SHAPES):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--iters", str(iters)], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:          # a shape that failed or hung: nothing more is started on the device
            print(json.dumps(dict(shape=name, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
