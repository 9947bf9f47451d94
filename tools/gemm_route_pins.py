#!/usr/bin/env python
"""One launch of every kernel family uvc_gemm_nt / uvc_gemm_tn select, at the smallest shape that selects it: the record of what a build LAUNCHES.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o pins -- python tools/gemm_route_pins.py        (one MI355X; no counters)
    python tools/gemm_route_pins.py --launches DIR > profiles/<build>_launches.txt                          (kernel, grid, workgroup, LDS per launch)
    python tools/gemm_route_pins.py --golden DIR > tests/golden/gemm_route_pins.json                        (problem -> kernel and template arguments)

Run on two builds, the two --launches lists must be identical where host code changed and kernels did not.  tests/test_gemm_route_cpu.py holds
uvc_gemm_nt_route / uvc_gemm_tn_route to the --golden file, without a GPU.  Only ops.gemm_nt / ops.gemm_tn are called, so the script runs on builds
older than the route queries.  The wide kernels go through force_generic 3 / 4 / 0x100 | ri, as tests/test_kernels_gpu.py runs them."""
import csv
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F32, BF16 = 0, 1
NONE, BIAS, BIAS_GELU, BIAS_RESID, BIAS_RESID_GATE, DGELU, BIAS_GELU_OUT, BIAS_GELU_GRAD, MUL_AUX, GELU_GRAD_Q8, MUL_AUX_Q8 = range(11)


def nt(M, N, K, epi=BIAS, fg=0, a_f32=0, c_f32=0, dtype=BF16, ln=0):
    return dict(call="nt", M=M, N=N, K=K, epilogue=epi, force_generic=fg, a_is_f32=a_f32, c_is_f32=c_f32, dtype=dtype, ln_out=ln)


def tn(M, N1, N2, variant=0, a_f32=0, dtype=BF16):
    return dict(call="tn", M=M, N1=N1, N2=N2, variant=variant, a_is_f32=a_f32, dtype=dtype)


PROBLEMS = [
    # generic 128 x 128: float32 mode, bf16 with float32 A, bf16 below every threshold, and forced
    nt(200, 72, 64, dtype=F32, a_f32=1, c_f32=1), nt(1100, 200, 72, a_f32=1), nt(1100, 200, 72, c_f32=1), nt(4096, 768, 192, fg=1),
    # row panels
    nt(1024, 192, 192), nt(16, 1000, 1024, a_f32=1, c_f32=1, epi=NONE),
    # K = 192 / 128 streaming: four / three waves x 64 columns, eight x 32 for the backward's multiplying epilogues, the one-byte GELU' pair
    nt(4096, 768, 192, epi=BIAS_GELU_GRAD), nt(4096, 320, 192), nt(4096, 256, 128, c_f32=1), nt(4096, 768, 192, a_f32=1),
    nt(4096, 768, 192, epi=MUL_AUX), nt(4096, 768, 192, epi=DGELU), nt(4096, 768, 192, epi=GELU_GRAD_Q8), nt(4096, 768, 192, epi=MUL_AUX_Q8),
    nt(4104, 192, 192, epi=BIAS_RESID),
    # K = 384 streaming: six waves, eight waves, six by force_generic = 5
    nt(4096, 384, 384), nt(4096, 768, 384), nt(4096, 768, 384, fg=5), nt(4096, 384, 384, c_f32=1, epi=BIAS_RESID),
    # N = 192 column-sliced: 32-row tiles, 16-row tiles, register-staged by force_generic = 2
    nt(4096, 192, 768), nt(4096, 192, 576, epi=NONE), nt(4096, 192, 512), nt(4096, 192, 256),
    nt(4096, 192, 768, c_f32=1), nt(4096, 192, 576, epi=BIAS_RESID), nt(4096, 192, 512, epi=BIAS_RESID_GATE), nt(4096, 192, 768, epi=BIAS_RESID, fg=2),
    # N = 192 on the LDS-DMA ring: K = 768 without and with ln_out, K = 512 / 256 / 192 with it, K = N = 192 without
    nt(4096, 192, 768, epi=BIAS_RESID), nt(4096, 192, 768, epi=BIAS_RESID_GATE, c_f32=1), nt(4096, 192, 768, epi=BIAS_RESID_GATE, ln=1),
    nt(4096, 192, 512, epi=BIAS_RESID, ln=1), nt(4096, 192, 256, epi=BIAS_RESID, c_f32=1, ln=1), nt(4096, 192, 192, epi=BIAS_RESID, ln=1),
    nt(4096, 192, 192, epi=BIAS_RESID), nt(4096, 192, 192, epi=BIAS_RESID, c_f32=1),
    # N = 384 with ln_out
    nt(4096, 384, 384, epi=BIAS_RESID, ln=1), nt(4096, 384, 768, epi=BIAS_RESID_GATE, ln=1),
    # 256 x 256: by shape (640 tiles), at any size by force_generic = 4 and = 3 (N >= 1792)
    nt(16129, 2560, 256), nt(512, 512, 256, fg=4, c_f32=1), nt(300, 1792, 256, fg=3),
    # 8-phase: by shape (few wide tiles, M >= 2048), force_generic = 3 (N < 1792), every tile height by 0x100 | ri, float32 C
    nt(2048, 768, 256), nt(300, 1536, 256, fg=3), nt(512, 512, 256, fg=0x108), nt(512, 512, 256, fg=0x106), nt(512, 512, 256, fg=0x105),
    nt(512, 512, 256, fg=0x104), nt(512, 512, 256, fg=0x100), nt(512, 512, 256, fg=0x104, c_f32=1),
    # TN: cfg 0 (float32 mode, bf16, float32 A), cfgs 1-5, the ring kernel by variant 2, 128 x 256 tiles by variant 3, float32 A on the big tiles
    tn(4096, 128, 64, dtype=F32, a_f32=1), tn(4096, 128, 64), tn(4096, 192, 192, a_f32=1),
    tn(4096, 192, 256), tn(4096, 256, 192), tn(4096, 384, 192), tn(4096, 192, 192), tn(4096, 768, 768),
    tn(4096, 192, 256, variant=1), tn(4096, 192, 256, variant=2), tn(4096, 256, 192, variant=2), tn(4096, 384, 192, variant=2), tn(4096, 768, 768, variant=2),
    tn(4096, 768, 768, variant=3), tn(4096, 192, 256, a_f32=1), tn(4096, 256, 192, a_f32=1), tn(4096, 384, 192, a_f32=1), tn(4096, 768, 768, a_f32=1),
]


def run():
    import torch
    from uvc_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    rnd = lambda *s, dt=torch.bfloat16: (torch.randn(*s, device=dev) * 0.1).to(dt)
    for i, p in enumerate(PROBLEMS):
        f32 = lambda flag: torch.float32 if flag else torch.bfloat16
        if p["call"] == "nt":
            M, N, K, e = p["M"], p["N"], p["K"], p["epilogue"]
            cdt = f32(p["c_is_f32"])
            q8 = e == GELU_GRAD_Q8
            kw = dict(bias=rnd(N, dt=torch.float32), C2=torch.empty(M, N, device=dev, dtype=cdt))
            if e in (BIAS_RESID, BIAS_RESID_GATE):
                kw.update(R=rnd(M, N, dt=cdt), R2=rnd(M, N, dt=cdt), gate=torch.tensor([0.3, 0.7], device=dev))
            if e in (DGELU, MUL_AUX, MUL_AUX_Q8):
                kw.update(aux=torch.randint(0, 255, (M, N), dtype=torch.uint8, device=dev) if e == MUL_AUX_Q8 else rnd(M, N, dt=f32(p["dtype"] == F32)))
            if p["ln_out"]:
                kw.update(ln_gamma=rnd(N, dt=torch.float32), ln_beta=rnd(N, dt=torch.float32), ln_out=torch.empty(M, N, device=dev, dtype=torch.bfloat16),
                          ln_mean=torch.empty(M, device=dev), ln_rstd=torch.empty(M, device=dev))
            Cm = torch.empty(M, N, device=dev, dtype=torch.uint8 if q8 else cdt)
            ops.gemm_nt(rnd(M, K, dt=f32(p["a_is_f32"])), rnd(N, K, dt=f32(p["dtype"] == F32)), Cm, dtype=p["dtype"], epilogue=e,
                        force_generic=p["force_generic"], **kw)
        else:
            M, N1, N2 = p["M"], p["N1"], p["N2"]
            ws = torch.empty(ops.gemm_tn_workspace_bytes(M, N1, N2), dtype=torch.uint8, device=dev)
            ops.gemm_tn(rnd(M, N1, dt=f32(p["a_is_f32"])), rnd(M, N2, dt=f32(p["dtype"] == F32)), torch.zeros(N1, N2, device=dev), ws, dtype=p["dtype"],
                        variant=p["variant"], colsum_out=torch.zeros(N1, device=dev))
        torch.cuda.synchronize()
        print("ran", i, json.dumps(p), flush=True)


def launches(d):
    """The trace's launches of the GEMM kernels (gemm*.hip) in dispatch order: (kernel, grid, workgroup, LDS bytes)."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Dispatch_Id"]))
    out = []
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        name = re.sub(r"\(.*$", "", name)           # the parameter list
        if not re.match(r"k_(gemm_|tn_reduce)", name):
            continue
        out.append((name, "x".join(r["Grid_Size_" + a] for a in "XYZ"), "x".join(r["Workgroup_Size_" + a] for a in "XYZ"), r["LDS_Block_Size"]))
    return out


def golden(d):
    ls = [l for l in launches(d) if not l[0].startswith("k_tn_reduce")]
    assert len(ls) == len(PROBLEMS), (len(ls), len(PROBLEMS))
    return [dict(p, kernel=l[0]) for p, l in zip(PROBLEMS, ls)]


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--launches":
        for l in launches(sys.argv[2]):
            print(" | ".join(l))
    elif len(sys.argv) > 2 and sys.argv[1] == "--golden":
        print("[\n" + ",\n".join(" " + json.dumps(e) for e in golden(sys.argv[2])) + "\n]")
    else:
        run()
