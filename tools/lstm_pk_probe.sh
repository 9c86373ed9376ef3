#!/bin/bash
# builds of the library whose encoder LSTM step (tools/lstm_pk_probe.hip, the product's lstm_step_fwd_kernel and its probe variants)
# is compiled WITH packed fp32 VALU ops (every other file as the product: without), in several forms of the kernel's hand-off from the
# v_pk_fma_f32 loop to the DPP reduction (L2S_LSTM_PROBE in tools/lstm_pk_probe.hip):
#   pk0 = as the compiler emits it, pk1 = + 16 wait states, pk2 = + a plain v_mov of every accumulator, pk3 = + an empty asm with the same constraints
# csrc/rnn_step.hip is built with -DL2S_LSTM_STEP_FWD_EXTERNAL (product flags), so that the probe object supplies l2s_lstm_step_fwd.
# Run here (cross-compiles); tools/lstm_pk_fuzz.sh runs tools/vgg_corun_fuzz.py on each on the GPU box.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
D=$R/tools/_lstm_pk; mkdir -p $D
OBJ=$R/lang2seg_amd/lib/obj
python $R/__graft_entry__.py > /dev/null
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result"
NOPK="-Xclang -target-feature -Xclang -packed-fp32-ops"
/opt/rocm/bin/hipcc $FL $NOPK -DL2S_LSTM_STEP_FWD_EXTERNAL -c $R/lang2seg_amd/csrc/rnn_step.hip -o $D/rnn_step_ext.o 2>/dev/null
for v in ${VARIANTS:-0 1 2 3 4 5 7}; do
  DEF=""; [ $v != 0 ] && DEF="-DL2S_LSTM_PROBE=$v"
  FLV="$FL"; [ $v = 9 ] && FLV="$FL $NOPK"      # probe 9: WITHOUT packed ops (the product's flags)
  /opt/rocm/bin/hipcc $FLV $DEF -c $R/tools/lstm_pk_probe.hip -o $D/lstm_pk$v.o 2>/dev/null
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $D/libpk$v.so $D/lstm_pk$v.o $D/rnn_step_ext.o $(ls $OBJ/*.o | grep -v '/rnn_step.o$')
  rm -f $D/lstm_pk$v.o
  /opt/rocm/bin/hipcc $FLV $DEF -S --cuda-device-only -o $D/lstm_pk$v.s $R/tools/lstm_pk_probe.hip 2>/dev/null
done
rm -f $D/rnn_step_ext.o
ls -la $D
