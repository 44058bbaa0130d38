#!/bin/bash
# Round-4 final check of the tree on the GPU box: the -m gpu suite, smoke()
# and the default bench line.
mkdir -p ${RR_OUT:-output}
timeout -k 10 420 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > ${RR_OUT:-output}/r4_final_tests.log 2>&1
rc=$?
tail -3 ${RR_OUT:-output}/r4_final_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > ${RR_OUT:-output}/r4_final_smoke.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full > ${RR_OUT:-output}/r4_final_bench.json 2> ${RR_OUT:-output}/r4_final_bench.err
