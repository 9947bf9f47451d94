#!/bin/bash
# Upper-bound probes for the two byte items VERDICT r3 next #5 asks to MEASURE before building (NOTEBOOK §11 / §12):
#   (a) teacher qkv projected inside its attention kernel   -> library variant "noteacherqkv": the no-grad forward (the teacher) skips its qkv GEMM
#       altogether (attention reads whatever the buffer holds): what the step would gain if that GEMM cost NOTHING
#   (b) fc1 stores ONE tensor instead of GELU(a) and GELU'(a) -> variant "onegelu": the training fc1 writes GELU(a) only, the backward reads the stale
#       GELU' buffer: same kernels, same reads, one 155-MB write per layer less -- what a one-tensor scheme would gain BEFORE paying for its recomputation
# Both variants compute wrong numbers on purpose; they are timing probes built from sed-edited COPIES of vit_engine.hip (the product source carries no switch).
#   (c) the weight-gradient partials reduced for free        -> variant "notnreduce": k_tn_reduce never launched
#   here:            tools/bound_probes.sh build   -> tools/perturb/libuvc_hip_{noteacherqkv,onegelu,notnreduce}.so
#   on the GPU box:  tools/bound_probes.sh run     -> gpurun_out/bound_probes.txt  (alternating same-box A/B through tools/exp_ab.sh)
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -Wno-unused-value -Wno-unused-result -I$R/include -I$R/uvc_amd/csrc"
if [ "${1:-}" = build ]; then
  python -m uvc_amd.build > /dev/null || exit 1
  mkdir -p /tmp/perturb "$R/tools/perturb"
  sed 's|^    TRY(nt(c, b.h1, 0, wmat(c, q\[2\], c.soff.blk_w\[l\]\[0\]), b.qkv, 0, d.M, 3 \* d.D, d.D,|    if (io->training) TRY(nt(c, b.h1, 0, wmat(c, q[2], c.soff.blk_w[l][0]), b.qkv, 0, d.M, 3 * d.D, d.D,|' "$R/uvc_amd/csrc/vit_engine.hip" > /tmp/perturb/vit_noteacherqkv.hip
  sed 's|TRY(nt(c, h2, 0, w1, ga, 0, rows, Fe, d.D, gp_q8(c, rows, Fe) ? UVC_EPI_BIAS_GELU_GRAD_Q8 : UVC_EPI_BIAS_GELU_GRAD, b1, nullptr, nullptr, nullptr, nullptr, gu));|TRY(nt(c, h2, 0, w1, gu, 0, rows, Fe, d.D, UVC_EPI_BIAS_GELU_OUT, b1));|' "$R/uvc_amd/csrc/vit_engine.hip" > /tmp/perturb/vit_onegelu.hip
  # (c) VERDICT r3 next #6: what ANY scheme that removes the weight-gradient partial reduction could gain -- the k_tn_reduce launches skipped altogether
  #     (the gradients stay unreduced: wrong numbers, same GEMMs)
  sed 's|^    k_tn_reduce<4><<<ceil_div(tot / 4, 256), 256, 0, st>>>|    if (false) k_tn_reduce<4><<<ceil_div(tot / 4, 256), 256, 0, st>>>|; s|^    k_tn_reduce<1><<<ceil_div(tot, 256), 256, 0, st>>>|    if (false) k_tn_reduce<1><<<ceil_div(tot, 256), 256, 0, st>>>|' "$R/uvc_amd/csrc/gemm_tn.hip" > /tmp/perturb/gemm_notnreduce.hip
  cmp -s /tmp/perturb/gemm_notnreduce.hip "$R/uvc_amd/csrc/gemm_tn.hip" &&{ echo "variant notnreduce did not apply"; exit 1; }
  sed -i 's|#include "gemm_common.h"|#include "'"$R"'/uvc_amd/csrc/gemm_common.h"|' /tmp/perturb/gemm_notnreduce.hip
  /opt/rocm/bin/hipcc $FLAGS -c /tmp/perturb/gemm_notnreduce.hip -o /tmp/perturb/gemm_notnreduce.o || exit 1
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/tools/perturb/libuvc_hip_notnreduce.so" $(ls "$R"/uvc_amd/csrc/build/*.o | grep -v '/gemm_tn.o$') /tmp/perturb/gemm_notnreduce.o || exit 1
  # (d) r6: GELU'(a) neither written by fc1 nor read by dfc2 (onegelu + the dgrad of fc2 without its multiply): the bound for any scheme that shrinks or
  #     recomputes that tensor (storing it in one byte gets half of this)
  sed 's|TRY(nt(c, h2, 0, w1, ga, 0, rows, Fe, d.D, gp_q8(c, rows, Fe) ? UVC_EPI_BIAS_GELU_GRAD_Q8 : UVC_EPI_BIAS_GELU_GRAD, b1, nullptr, nullptr, nullptr, nullptr, gu));|TRY(nt(c, h2, 0, w1, gu, 0, rows, Fe, d.D, UVC_EPI_BIAS_GELU_OUT, b1));|; s|TRY(nt(c, gA, gf, sh(c, so.blk_wt\[l\]\[3\]), dA, 0, rows, d.F, d.D, gp_q8(c, rows, d.F) ? UVC_EPI_MUL_AUX_Q8 : UVC_EPI_MUL_AUX, nullptr, nullptr, nullptr, fa, nullptr,$|TRY(nt(c, gA, gf, sh(c, so.blk_wt[l][3]), dA, 0, rows, d.F, d.D, UVC_EPI_NONE, nullptr, nullptr, nullptr, nullptr, nullptr,|' "$R/uvc_amd/csrc/vit_engine.hip" > /tmp/perturb/vit_nogp.hip
  grep -q "dA, 0, rows, d.F, d.D, UVC_EPI_NONE, nullptr, nullptr, nullptr, nullptr, nullptr,$" /tmp/perturb/vit_nogp.hip || { echo "variant nogp did not apply"; exit 1; }
  for v in noteacherqkv onegelu nogp; do
    # (r6: the teacher's qkv GEMM no longer exists as a launch -- k_qkv_attn_fwd -- so `noteacherqkv` does not apply at DeiT-Tiny's shape any more: skipped)
    cmp -s /tmp/perturb/vit_$v.hip "$R/uvc_amd/csrc/vit_engine.hip" && { echo "variant $v does not apply to the current engine: skipped"; continue; }
    sed -i 's|#include "common.h"|#include "'"$R"'/uvc_amd/csrc/common.h"|; s|#include "../../include/|#include "'"$R"'/include/|' /tmp/perturb/vit_$v.hip
    /opt/rocm/bin/hipcc $FLAGS -c /tmp/perturb/vit_$v.hip -o /tmp/perturb/vit_$v.o || exit 1
    objs=$(ls "$R"/uvc_amd/csrc/build/*.o | grep -v '/vit_engine.o$')
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/tools/perturb/libuvc_hip_$v.so" $objs /tmp/perturb/vit_$v.o || exit 1
  done
  ls -la "$R/tools/perturb"
  exit 0
fi
OUT=$R/gpurun_out/bound_probes.txt
mkdir -p "$R/gpurun_out"
export GRAFT_REPO_ROOT=${GRAFT_REPO_ROOT:-$R}
{
  echo "# same-box alternating A/B, DeiT-Tiny batch 512, 60 steps each: <variant> <img/s> <ms per step> <sum of stand-alone kernel ms>"
  for v in ${PROBES:-onegelu nogp notnreduce}; do echo "## $v"; bash "$R/tools/exp_ab.sh" $v; done
} > "$OUT" 2>&1
cat "$OUT"
