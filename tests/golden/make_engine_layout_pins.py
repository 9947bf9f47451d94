#!/usr/bin/env python3
"""Record what the engines' host-side queries answer into tests/golden/engine_layout_pins.json: the parameter / shadow layouts, the
workspace sizes and the frozen ranges of the compact entry points, and the dense engine's layout, workspace sizes and workspace
offsets (include/uvc_vit.h).  Pure host code: no GPU.  Run it on the library built at the commit whose answers are to be pinned --
BEFORE the engines' host code is restructured; tests/test_engine_layout_pins_cpu.py compares a later build against the file.

    python tests/golden/make_engine_layout_pins.py
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

BATCHES = (2, 7)
# name -> uvc_vit_cfg fields (dtype: 0 float32, 1 bf16) and the (heads, v_dim, hidden) of every compact block
CASES = {
    # every branch of a block: both, MLP only, heads only, neither; distillation token
    "d128_mixed_bf16": dict(cfg=dict(img_size=32, patch_size=16, in_chans=3, num_classes=16, embed_dim=128, depth=4, num_heads=2, hidden=512,
                                     ntok=2, dtype=1), blocks=[(2, 64, 512), (0, 0, 256), (1, 16, 0), (0, 0, 0)]),
    # the same with float32 residual rows: the eval entry accepts it, training refuses
    "d128_mixed_bf16_f32resid": dict(cfg=dict(img_size=32, patch_size=16, in_chans=3, num_classes=16, embed_dim=128, depth=4, num_heads=2,
                                              hidden=512, ntok=2, dtype=1, resid_f32=1), blocks=[(2, 64, 512), (0, 0, 256), (1, 16, 0), (0, 0, 0)]),
    # every value width
    "d192_vdims_bf16": dict(cfg=dict(img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=192, depth=12, num_heads=3, hidden=768,
                                     ntok=2, dtype=1), blocks=[(3, 16, 768), (2, 32, 384), (1, 48, 192), (3, 64, 64)]),
    "d192_vdims_fp32": dict(cfg=dict(img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=192, depth=12, num_heads=3, hidden=768,
                                     ntok=1, dtype=0), blocks=[(3, 16, 768), (2, 32, 384), (1, 48, 192), (3, 64, 64)]),
    "d128_no_blocks": dict(cfg=dict(img_size=32, patch_size=16, in_chans=3, num_classes=16, embed_dim=128, depth=4, num_heads=2, hidden=512,
                                    ntok=1, dtype=1), blocks=[]),
    # 577 tokens: eval runs it, training answers UVC_ERR_UNSUPPORTED
    "d192_384px_bf16": dict(cfg=dict(img_size=384, patch_size=16, in_chans=3, num_classes=1000, embed_dim=192, depth=12, num_heads=3, hidden=768,
                                     ntok=1, dtype=1), blocks=[(3, 48, 384), (2, 32, 192)]),
}


def plain(v):
    """A ctypes structure / array as nested lists and ints."""
    if isinstance(v, C.Structure):
        return {n: plain(getattr(v, n)) for n, _ in v._fields_}
    if isinstance(v, C.Array):
        return [plain(e) for e in v]
    return int(v)


def bind():
    from uvc_amd import compact_train as CT
    from uvc_amd import model_distilled as MD
    CT._bind()
    lib = MD._bind()
    lib.uvc_vit_ws_offsets.argtypes = [C.POINTER(MD.uvc_vit_cfg), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.uvc_vit_ws_offsets.restype = C.c_int
    return lib


def query(lib, case):
    """Everything the host-side entry points answer for one case, as JSON-able values (return codes included)."""
    from uvc_amd import _lib as L
    from uvc_amd import model_distilled as MD
    cfg = MD.uvc_vit_cfg()
    for k, v in case["cfg"].items():
        setattr(cfg, k, v)
    nb = len(case["blocks"])
    blocks = (L.uvc_compact_block * max(1, nb))()
    for k, (h, dv, f) in enumerate(case["blocks"]):
        blocks[k].heads, blocks[k].v_dim, blocks[k].hidden = h, dv, f
    out = {}
    for name, fn in (("compact_layout", lib.uvc_vit_compact_layout), ("compact_train_layout", lib.uvc_vit_compact_train_layout)):
        off, soff = MD.uvc_vit_offsets(), MD.uvc_vit_shadow_offsets()
        rc = fn(C.byref(cfg), blocks, nb, C.byref(off), C.byref(soff))
        out[name] = dict(rc=rc, offsets=plain(off), shadow_offsets=plain(soff)) if rc == 0 else dict(rc=rc)
    out["compact_workspace_bytes"] = [int(lib.uvc_vit_compact_workspace_bytes(C.byref(cfg), blocks, nb, B)) for B in BATCHES]
    out["compact_train_workspace_bytes"] = [int(lib.uvc_vit_compact_train_workspace_bytes(C.byref(cfg), blocks, nb, B)) for B in BATCHES]
    cap = 2 * max(1, nb)
    ranges, cnt = (C.c_int64 * (2 * cap))(), C.c_int32()
    rc = lib.uvc_vit_compact_frozen_ranges(C.byref(cfg), blocks, nb, ranges, cap, C.byref(cnt))
    out["compact_frozen_ranges"] = dict(rc=rc, ranges=[[int(ranges[2 * i]), int(ranges[2 * i + 1])] for i in range(cnt.value)])
    # the dense engine at the same cfg
    off, soff = MD.uvc_vit_offsets(), MD.uvc_vit_shadow_offsets()
    rc = lib.uvc_vit_layout(C.byref(cfg), C.byref(off), C.byref(soff))
    out["layout"] = dict(rc=rc, offsets=plain(off), shadow_offsets=plain(soff))
    out["workspace_bytes"] = [[int(lib.uvc_vit_workspace_bytes(C.byref(cfg), B, mode)) for mode in (0, 1, 2)] for B in BATCHES]
    wso = []
    for B in BATCHES:
        for mode in (0, 1, 2):
            pe, dpe = C.c_int64(), C.c_int64()
            rc = lib.uvc_vit_ws_offsets(C.byref(cfg), B, mode, C.byref(pe), C.byref(dpe))
            wso.append([rc, int(pe.value), int(dpe.value)])
    out["ws_offsets"] = wso
    return out


def main():
    lib = bind()
    pins = {name: query(lib, case) for name, case in CASES.items()}
    with open(os.path.join(HERE, "engine_layout_pins.json"), "w") as f:
        json.dump(pins, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(len(pins), "cases")


if __name__ == "__main__":
    main()
