#!/bin/bash
# libk5's GEMM against the vendor library on the model's shapes, same box, alternating, NO monitor kernel (a persistent 256-workgroup launch loses a
# CU to it and runs two rounds).  libk5 with the plain bf16 store the vendor call does.   tools/vendor_ab.sh
R=$PWD
for round in 1 2; do
  python $R/tools/blaslt_ref.py 2>/dev/null | grep -E "qk|out|ff1|ff2"
  for s in "47616 3584 1792" "47616 1792 1792" "47616 7168 1792" "47616 1792 7168"; do
    python $R/tools/gemm_time.py $s 20 2>/dev/null | sed "s/^/libk5    /"
  done
done
