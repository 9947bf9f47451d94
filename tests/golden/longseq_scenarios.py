"""Long-sequence scenarios (N > 256): micro models with 4-pixel patches at 64 / 96 / 112 px (N = 257, 577 / 578, 785) and the
Stage-2 micro scenario at N = 577.  recipe() / stage2_recipe() build them as scenarios.py builds its own; register() adds them to
scenarios.py's tables for make_golden.run_scenario (called by make_golden_longseq.py only: the tests' own scenario lists stay as they are)."""
import scenarios as SC

LONG_MODELS = {
    f"micro_p4_{s}": dict(img_size=s, patch_size=4, num_classes=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, enable_dist=0, weight_gain=3.0)
    for s in (64, 96, 112)
}
LONG_MODELS["micro_p4_96_dist"] = dict(LONG_MODELS["micro_p4_96"], enable_dist=1)
LONG_MODELS["deit_tiny_384"] = dict(SC.MODELS["deit_tiny"], img_size=384)

# Stage-1: the micro scenarios' settings (pruned primal-dual state; patch gating off, mode 1, mode 2) on the long-sequence models
LONG_SCENARIOS = {}
for s in (64, 96, 112):
    LONG_SCENARIOS[f"longseq_p4_{s}_pruned"] = dict(model=f"micro_p4_{s}", batch=4, steps=1, warmup=0, state="pruned", seed=60 + s)
    LONG_SCENARIOS[f"longseq_p4_{s}_patch1"] = dict(model=f"micro_p4_{s}", batch=4, steps=1, warmup=0, state="pruned", seed=61 + s,
                                                    gating_interval=2, enable_patch_gating=1)
    LONG_SCENARIOS[f"longseq_p4_{s}_patch2"] = dict(model=f"micro_p4_{s}", batch=4, steps=1, warmup=0, state="pruned", seed=62 + s,
                                                    gating_interval=2, enable_patch_gating=2, patch_tau=0.7)
LONG_SCENARIOS["longseq_p4_96_deit"] = dict(model="micro_p4_96_dist", batch=4, steps=1, warmup=0, state="pruned", seed=170)
LONG_SCENARIOS["longseq_tiny384"] = dict(model="deit_tiny_384", batch=2, steps=1, warmup=0, state="pruned", seed=171,
                                         gating_interval=2, warmup_steps=1)

LONG_STAGE2 = {
    "stage2_longseq_p4_96": dict(model="micro_p4_96", batch=4, steps=1, seed=172, skip_blocks=[], epoch_of_step=[1]),
}



def _model(r):
    r["model_cfg"] = dict(LONG_MODELS[r["model"]])
    return r


def recipe(name: str) -> dict:
    r = dict(SC.DEFAULTS)
    r.update(LONG_SCENARIOS[name])
    r["name"] = name
    return _model(r)


def stage2_recipe(name: str) -> dict:
    r = dict(SC.STAGE2_DEFAULTS)
    r.update(LONG_STAGE2[name])
    r["name"] = name
    return _model(r)


def register():
    SC.MODELS.update(LONG_MODELS)
    SC.SCENARIOS.update(LONG_SCENARIOS)
    SC.STAGE2.update(LONG_STAGE2)
