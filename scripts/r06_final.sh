#!/bin/bash
# On the GPU box: the round's closing run - full GPU suite, smoke, the --full bench line, the driver's form with --full, kernel stats of
# the plain run.  usage: OUT_DIR=<dir> scripts/r06_final.sh
out=${OUT_DIR:?set OUT_DIR to the directory for the records}
export PYTHONPATH=$PWD
R=$PWD
mkdir -p $out
out=$(cd $out && pwd)  # (absolute: the rocprofv3 pass below runs from /tmp)
timeout 1500 python -m pytest tests -m gpu -x -q > $out/pytest_final.txt 2>&1
grep -E "passed|failed|error" $out/pytest_final.txt | tail -2
python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke_final.txt 2>&1; tail -2 $out/smoke_final.txt
python bench.py --full > $out/bench_final.json 2> $out/bench_final.err
python bench.py --full --steps 20 --warmup 5 > $out/bench_driver_form_final.json 2> $out/bench_driver_form_final.err
python - "$out" <<'P'
import json, sys
for f in ("bench_final", "bench_driver_form_final"):
    for l in open("%s/%s.json" % (sys.argv[1], f)):
        if l.startswith("{"):
            j = json.loads(l)
            print(f, round(j["value"], 1), j["roofline"]["frac"], j["roofline"]["achieved"], j.get("value_ref_shape"), j.get("value_session_loop"), j["cpu_baseline"]["value"])
P
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $out/stats_final -o r --output-format csv -- python $R/bench.py --no-cpu-baseline --no-kernel-pass --no-full-leg --no-pmc --no-config-legs --no-session-leg > /dev/null 2> $out/stats_final.err
ls $out/stats_final | head
