#!/bin/bash
# Shows once that tests/test_streaming_batch_gpu.py (r3) and tests/test_wide_models_gpu.py (r4) go red when a production kernel is wrong.
#   here (build container):  tools/perturb_demo.sh build     -> tools/perturb/libuvc_hip_{ws,lnbwd,wide,row384,tn8p,row384fwd}.so (git-ignored; they travel with gpurun)
#   on the GPU box:          tools/perturb_demo.sh run       -> gpurun_out/perturb_demo.txt
# The perturbed libraries are built from sed-edited COPIES of the file that holds the kernel (gemm_nt_ws.hip for k_gemm_ws, gemm_nt_lnbwd.hip for lnbwd, gemm_nt_wide.hip for wide / row384 / row384fwd, gemm_tn.hip for tn8p) under /tmp:
# the product source carries no test switch.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -Wno-unused-value -Wno-unused-result -I$R/include -I$R/uvc_amd/csrc"
if [ "${1:-}" = build ]; then
  python -m uvc_amd.build > /dev/null || exit 1
  mkdir -p /tmp/perturb "$R/tools/perturb"
  # 1. k_gemm_ws: every output tile of the K <= 192 streaming GEMM (qkv, fc1, dfc2, dproj) scaled by 1.02
  sed 's|\*reinterpret_cast<f32x4\*>(stg + li \* EPW + j \* 16 + gq \* 4) = c;|*reinterpret_cast<f32x4*>(stg + li * EPW + j * 16 + gq * 4) = c * 1.02f;|' "$R/uvc_amd/csrc/gemm_nt_ws.hip" > /tmp/perturb/gemm_ws.hip
  # 2. k_gemm_wsn_lnbwd_dma: dx of the fused dgrad + LayerNorm backward scaled by 1.02
  sed 's|o\[e\] = rstd \* (c0\[e\] - c1 - xh \* c2);   |o[e] = 1.02f * rstd * (c0[e] - c1 - xh * c2);   |' "$R/uvc_amd/csrc/gemm_nt_lnbwd.hip" > /tmp/perturb/gemm_lnbwd.hip
  # 3. (r4) the wide-tile NT kernels of DeiT-Small / Base (k_gemm_nt256 and k_gemm_nt8p share NT_EPILOGUE_TILE): staged accumulator x 1.02
  sed 's|(stg_at<true>(stg, lane \& 15, j \* 4 + (lane >> 4))) = acc\[h\]\[j\];  |(stg_at<true>(stg, lane \& 15, j * 4 + (lane >> 4))) = acc[h][j] * 1.02f;|' "$R/uvc_amd/csrc/gemm_nt_wide.hip" > /tmp/perturb/gemm_wide.hip
  # 4. (r4) k_gemm_row384_lnbwd (D = 384 dgrad + LayerNorm backward on a row tile): dx x 1.02
  sed 's|o\[e\] = R.rstd \* (gy\[i\]\[e\] - c1 - ((xv\[i\]\[e\] - R.mean) \* R.rstd) \* c2);|o[e] = 1.02f * R.rstd * (gy[i][e] - c1 - ((xv[i][e] - R.mean) * R.rstd) * c2);|' "$R/uvc_amd/csrc/gemm_nt_wide.hip" > /tmp/perturb/gemm_row384.hip
  # 5. (r4) k_gemm_tn8p (256 x 256 weight-gradient tiles of DeiT-Base): partial tile x 1.03
  python3 - "$R/uvc_amd/csrc/gemm_tn.hip" /tmp/perturb/gemm_tn8p.hip <<'PY'
import sys
s = open(sys.argv[1]).read()
i = s.index("void k_gemm_tn8p(TnArgs g)")
j = s.index("*reinterpret_cast<f32x4*>(P + (size_t)n1 * g.N2 + n2) = acc[i][j];", i)
s = s[:j] + "*reinterpret_cast<f32x4*>(P + (size_t)n1 * g.N2 + n2) = acc[i][j] * 1.03f;" + s[j + len("*reinterpret_cast<f32x4*>(P + (size_t)n1 * g.N2 + n2) = acc[i][j];"):]
open(sys.argv[2], "w").write(s)
PY
  # 6. (r4) k_gemm_row384_lnbwd<.., 1> (D = 384: fc2 / attn.proj + residual + the next LayerNorm in one launch): the GEMM result x 1.02 before bias / residual
  sed 's|float t = epi_scale_bias(v\[i\]\[e\], 1.0f, bv\[e\]);|float t = epi_scale_bias(v[i][e] * 1.02f, 1.0f, bv[e]);|' "$R/uvc_amd/csrc/gemm_nt_wide.hip" > /tmp/perturb/gemm_row384fwd.hip
  for v in ws lnbwd wide row384 tn8p row384fwd; do
    case $v in      # the file the variant is a copy of: its object is the one the perturbed object replaces
      ws) src=gemm_nt_ws ;; lnbwd) src=gemm_nt_lnbwd ;; tn8p) src=gemm_tn ;; *) src=gemm_nt_wide ;;
    esac
    cmp -s /tmp/perturb/gemm_$v.hip "$R/uvc_amd/csrc/$src.hip" && { echo "perturbation $v did not apply"; exit 1; }
    sed -i 's|#include "gemm_common.h"|#include "'"$R"'/uvc_amd/csrc/gemm_common.h"|' /tmp/perturb/gemm_$v.hip
    /opt/rocm/bin/hipcc $FLAGS -c /tmp/perturb/gemm_$v.hip -o /tmp/perturb/gemm_$v.o || exit 1
    objs=$(ls "$R"/uvc_amd/csrc/build/*.o | grep -v "/$src.o\$")
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/tools/perturb/libuvc_hip_$v.so" $objs /tmp/perturb/gemm_$v.o || exit 1
  done
  ls -la "$R/tools/perturb"
  exit 0
fi
OUT=$R/gpurun_out/perturb_demo.txt
mkdir -p "$R/gpurun_out"
cp "$R/uvc_amd/libuvc_hip.so" /tmp/libuvc_hip_good.so
{
  echo "# tests/test_streaming_batch_gpu.py::test_tiny_step_matches_oracle_at_streaming_batch with one streaming kernel perturbed (tools/perturb_demo.sh)"
  for v in ws lnbwd; do
    cp "$R/tools/perturb/libuvc_hip_$v.so" "$R/uvc_amd/libuvc_hip.so"
    echo; echo "## perturbed: $v (k_gemm_ws output x 1.02 | k_gemm_wsn_lnbwd_dma dx x 1.02) -- expected: FAILED"
    (cd "$R" && python -m pytest tests/test_streaming_batch_gpu.py -q -x -k "matches_oracle_at_streaming_batch and not fp32" 2>&1 > /tmp/perturb_out.txt 2>&1; grep -E "AssertionError|assert " /tmp/perturb_out.txt | cut -c1-600 | head -6; grep -E "^[0-9]+ (passed|failed)|[0-9]+ failed|[0-9]+ passed" /tmp/perturb_out.txt | tail -1)
  done
  echo; echo "# tests/test_wide_models_gpu.py::test_wide_model_step_matches_oracle_on_production_kernels (DeiT-Small batch 24, DeiT-Base batch 12 with the wide tiles forced)"
  for v in wide row384 tn8p row384fwd; do
    cp "$R/tools/perturb/libuvc_hip_$v.so" "$R/uvc_amd/libuvc_hip.so"
    echo; echo "## perturbed: $v (wide NT tiles x 1.02 | k_gemm_row384_lnbwd dx x 1.02 | k_gemm_row384_lnbwd<.., 1> (forward + LayerNorm) GEMM result x 1.02 | k_gemm_tn8p partial tiles x 1.03 (a leaf kernel: below the 2.5 % per-tensor bound a scaling is inside the bf16 noise the bound admits)) -- expected: FAILED"
    (cd "$R" && python -m pytest tests/test_wide_models_gpu.py -q -k "matches_oracle_on_production_kernels" 2>&1 > /tmp/perturb_out.txt 2>&1; grep -E "AssertionError|assert " /tmp/perturb_out.txt | cut -c1-600 | head -6; grep -E "^[0-9]+ (passed|failed)|[0-9]+ failed|[0-9]+ passed" /tmp/perturb_out.txt | tail -1)
  done
  cp /tmp/libuvc_hip_good.so "$R/uvc_amd/libuvc_hip.so"
  echo; echo "## unperturbed library -- expected: passed"
  (cd "$R" && python -m pytest tests/test_streaming_batch_gpu.py -q -x -k "matches_oracle_at_streaming_batch and not fp32" 2>&1 | grep -E "passed|failed")
  (cd "$R" && python -m pytest tests/test_wide_models_gpu.py -q -k "matches_oracle_on_production_kernels" 2>&1 | grep -E "passed|failed")
} > "$OUT" 2>&1
cat "$OUT"
