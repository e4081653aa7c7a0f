#!/bin/bash
# Round evidence on the GPU box, one call: the whole -m gpu suite, every bench line, the backward flavours, the iteration leg, the
# reference call pattern's profile, rocprofv3 kernel stats (pipelined + serial command) and the PMC passes.  Everything lands under
# $TEXGS_OUT (default out/); copy what is to be judged to profiles/.
R=$(cd "$(dirname "$0")/.." && pwd)
export TEXGS_OUT=${TEXGS_OUT:-$R/out}
O=$TEXGS_OUT
cd "$R"
mkdir -p "$O"
T0=$(date +%s)
rm -f gpurun_out/parity_report.jsonl
timeout 1500 python -m pytest tests -m gpu -q -rA --durations=15 -p no:cacheprovider 2>&1 | grep -E "passed|failed|PASSED|FAILED|ERROR|rror|^[0-9.]+s (call|setup)" | tail -160 > $O/gpu_tests.log
tail -3 $O/gpu_tests.log; grep -E "^FAILED|^ERROR" $O/gpu_tests.log | head
echo "[tests $(( $(date +%s) - T0 )) s]"
# the PMC traffic pass first: the bench lines below then carry roofline.traffic of THESE kernel sources
bash scripts/prof.sh > $O/prof.log 2>&1
python scripts/prof_summary.py $O/prof > $O/prof_summary.txt 2>&1
python scripts/make_traffic.py $O/prof $O/traffic.json > /dev/null 2>&1
cp $O/traffic.json profiles/r06_traffic.json
echo "[prof $(( $(date +%s) - T0 )) s]"
timeout 600 python bench.py --full > $O/bench_c3.json 2> $O/bench_c3.err
timeout 300 python bench.py --full --streams 1 --no-cpu-baseline > $O/bench_c3_serial.json 2> $O/bench_c3_serial.err
timeout 300 python bench.py --full --streams 4 --no-cpu-baseline --no-kernel-table > $O/bench_c3_s4.json 2> $O/bench_c3_s4.err
timeout 300 python bench.py --full --prefetch 0 --no-cpu-baseline --no-kernel-table --no-extra-legs > $O/bench_c3_noprefetch.json 2> $O/bench_c3_noprefetch.err
timeout 300 python bench.py --full --no-cpu-baseline --no-kernel-table --no-extra-legs > $O/bench_c3_again.json 2> $O/bench_c3_again.err
timeout 300 python bench.py --full --workload c2 --no-cpu-baseline > $O/bench_c2.json 2> $O/bench_c2.err
timeout 300 python bench.py --full --workload c5 --no-cpu-baseline --steps 8 --warmup 3 > $O/bench_c5.json 2> $O/bench_c5.err
timeout 300 python bench.py --full --surface diff_gauss --no-cpu-baseline > $O/bench_c3_diff_gauss.json 2> $O/bench_c3_diff_gauss.err
TEXGS_FORCE_DIST=1 RANK=0 LOCAL_RANK=0 WORLD_SIZE=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29533 timeout 300 python bench.py --full --no-cpu-baseline --no-kernel-table > $O/bench_c3_rccl1.json 2> $O/bench_c3_rccl1.err
timeout 300 python scripts/bench_variants.py > $O/variants.jsonl 2> $O/variants.err
timeout 300 python bench.py --leg iteration --steps 10 --warmup 3 > $O/bench_iteration_mixed.json 2> $O/bench_iteration_mixed.err
TEXGS_UV_PRECISION=fp32 timeout 300 python bench.py --leg iteration --steps 10 --warmup 3 > $O/bench_iteration_fp32.json 2> $O/bench_iteration_fp32.err
# the C3 geometry with a 302 MB texture (past the 256 MB Infinity Cache), serial and pipelined, beside R = 1024
timeout 300 python bench.py --full --tex-res 2048 --no-cpu-baseline --no-extra-legs > $O/bench_c3_R2048.json 2> $O/bench_c3_R2048.err
timeout 300 python bench.py --full --tex-res 2048 --streams 1 --no-cpu-baseline --no-extra-legs > $O/bench_c3_R2048_serial.json 2> $O/bench_c3_R2048_serial.err
echo "[bench $(( $(date +%s) - T0 )) s]"
bash scripts/prof_ref_pattern.sh > $O/ref_pattern_profile.txt 2>&1
echo "[ref pattern $(( $(date +%s) - T0 )) s]"
bash scripts/prof_iteration.sh > $O/iteration_profile.txt 2>&1
echo "[iteration profile $(( $(date +%s) - T0 )) s]"
bash scripts/prof_uv_backward.sh > $O/uv_kernels_profile.txt 2>&1
echo "[uv kernels profile $(( $(date +%s) - T0 )) s]"
# the raw per-launch traces and counter tables are large and have been summarised above -- drop them
find $O -name "*kernel_trace.csv" -delete; find $O -name "*counter_collection.csv" -delete
find $O -name "*agent_info.csv" -delete; find $O -name "*.db" -delete; find $O -name "*.rocpd" -delete
du -sh $O | tail -1
python - <<'PY'
import json, os
O = os.environ["TEXGS_OUT"]
for n in ("c3", "c3_again", "c3_noprefetch", "c3_serial", "c3_s4", "c2", "c5", "c3_diff_gauss", "c3_rccl1", "c3_R2048", "c3_R2048_serial"):
    try:
        j = json.loads([l for l in open(f"{O}/bench_{n}.json").read().splitlines() if l.startswith("{")][-1])
        print(n, j["value"], j.get("value_long"), j["ms_per_step_percentiles"]["median"], {k: round(v["avg_us"]) for k, v in j["kernels"].items()},
              "cpu", (j.get("cpu_baseline") or {}).get("value"), "frac", (j.get("roofline") or {}).get("frac"), (j.get("roofline") or {}).get("solo_frac"),
              (j.get("roofline") or {}).get("frac_survey_8d"))
        for k in ("reference_call_pattern", "reference_iteration", "retexture_pattern"):
            if j.get(k): print("   ", k, {a: b for a, b in j[k].items() if a != "note"})
        if j["config"].get("grad_allreduce_measured"): print("   ", j["config"]["grad_allreduce_measured"])
    except Exception as e:
        print(n, "ERR", e, open(f"{O}/bench_{n}.err").read()[-800:])
for n in ("mixed", "fp32"):
    try:
        j = json.loads([l for l in open(f"{O}/bench_iteration_{n}.json").read().splitlines() if l.startswith("{")][-1])
        print("iteration", n, j["uv_per_render_ms_per_iteration"], j["uv_once_ms_per_iteration"], j["split_uv_once_ms"], j["rasterizer_kernels_us_per_iteration"], j.get("uvnet_backward_us"))
    except Exception as e:
        print("iteration", n, "ERR", e, open(f"{O}/bench_iteration_{n}.err").read()[-800:])
PY
cat $O/variants.jsonl | cut -c1-400
cat $O/ref_pattern_profile.txt | head -50
cat $O/iteration_profile.txt | head -34
grep -E "k_uv_backward|uv_backward_" $O/uv_kernels_profile.txt | cut -c1-420
grep -E "k_render|k_texgrad|k_preprocess|k_bin_off|k_radix|k_depth|k_dup|k_ranges|k_tile" $O/prof_summary.txt | grep calls | head -40
cat $O/traffic.json | head -40
