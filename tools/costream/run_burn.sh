#!/bin/bash
# GPU box: every product kernel as a victim next to the pure-register matrix-instruction burner (debug library) - is anything but the matrix
# instructions needed?  usage: TABLE="1 2 5" tools/costream/run_burn.sh  (burner kinds: csrc/debug/waymodet_debug.h)
cd "$(dirname "$0")/../.."
O=gpurun_out/r06_costream
mkdir -p $O
export WT_LIB_PATH=$PWD/waymo_2d_tracking_amd/csrc/libwaymotrack_debug.so WT_EXPERIMENT=1
for k in $TABLE; do echo "== all victims next to burn kind $k"; AGGRESSOR=burn$k timeout 900 python tools/costream/victims_table.py 2>&1 | grep -v amdgpu.ids | tail -30; done > $O/burn_table.txt 2>&1
