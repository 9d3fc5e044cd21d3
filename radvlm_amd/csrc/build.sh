#!/bin/bash
# Build libradvlm_hip.so (gfx950) in-tree. hipcc cross-compiles without a GPU.
#   build.sh [out.so [flags...]]   variant build: every source again with the extra flags (e.g. -DRV_ATTN_STAMPS), objects in build/<out>/ (lib_S.so: build/lib_S/),
#                                  library radvlm_amd/<out.so> (load it with RADVLM_HIP_LIB); the default build's objects stay as they are
# The compiler's per-kernel resource report is kept (build/*.res) and the default build FAILS if a kernel of any source in SRCS touches
# scratch memory: a rolled epilogue loop once turned the GEMM accumulators into a scratch array and cost 18 % unnoticed.
set -e
cd "$(dirname "$0")"
SRCS="gemm_bf16 attention ops gemv decode lora_merge extend sample beam lookup kvq cfg prefix score dola constrain policy preference lora_decode attn_probs kvpress adam8 distill spec nf4"
OUT=${1:-libradvlm_hip.so}
VARFLAGS="${*:2}"
OBJ=build; [ $# -gt 0 ] && OBJ=build/${OUT%.so}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I. -I../../include -Wno-unused-result -Rpass-analysis=kernel-resource-usage"
mkdir -p $OBJ
pids=()
# attention.hip: no SLP vectorisation -- hipcc packs adjacent fp32 adds / multiplies of the softmax and dS arithmetic into v_pk_*_f32, which is slower
# than the two scalar instructions beside MFMAs (guide: "an anti-lever beside MFMAs"; same-box A/B profiles/r04_ab_attn_no_slp_merged_waits.txt).
# The variant flags come last, so a variant can turn it back on (-fslp-vectorize).
for f in $SRCS; do
  EXTRA=""; [ $f = attention ] && EXTRA="-fno-slp-vectorize"
  ( hipcc $FLAGS $EXTRA $VARFLAGS -c $f.hip -o $OBJ/$f.o 2> $OBJ/$f.res || { cat $OBJ/$f.res >&2; exit 1; } ) &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
grep -h "error\|warning" $OBJ/*.res | grep -v "Rpass" | head -20 || true
if grep -h -B8 "ScratchSize \[bytes/lane\]: [1-9]" $(printf "$OBJ/%s.res " $SRCS) | grep "Function Name"; then
  # a variant may spill on purpose (the in-kernel cycle stamps of -DRV_STAMPS do): it is only told
  if [ $# -gt 0 ]; then echo "WARNING: the kernels above use scratch memory (see $OBJ/*.res)" >&2
  else echo "ERROR: the kernels above use scratch memory (see $OBJ/*.res)" >&2; exit 1; fi
fi
hipcc --offload-arch=gfx950 -shared -fPIC $(printf "$OBJ/%s.o " $SRCS) -o ../$OUT
echo "built radvlm_amd/$OUT"
