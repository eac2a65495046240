#!/bin/bash
# Round-4 end measurements.  Everything lands in gpurun_out/final4/ (copied to profiles/r04_*).  PMC passes first: the bench lines
# read the traffic files they produce (bench.py / scripts/_train_bench.py look for profiles/r04_pmc_*_traffic.json).
# SECTIONS="rexnet" (or any subset of: headline rexnet yolov4 fp8 mobileone misc) re-measures one configuration after a change to its kernels.
R=${GRAFT_REPO_ROOT:-/root/repo}; cd $R; O=$R/gpurun_out/final4; mkdir -p $O
SECTIONS=${SECTIONS:-"headline rexnet yolov4 fp8 mobileone misc"}
want() { case " $SECTIONS " in *" $1 "*) return 0;; esac; return 1; }
[ "$SECTIONS" = "headline rexnet yolov4 fp8 mobileone misc" ] && rm -rf $O/*
summ() {  # summ <trace dir> <out prefix> <header>
python - "$1" "$2" "$3" <<'PY'
import csv, glob, sys, collections
d, out, header = sys.argv[1], sys.argv[2], sys.argv[3]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
per, grid, tot = collections.defaultdict(lambda: [0, 0]), collections.defaultdict(lambda: [0, 0]), 0
for r in csv.DictReader(open(f)):
    t = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
    name = (name[:name.index("(")] if "(" in name else name)[:110]
    per[name][0] += 1; per[name][1] += t
    k = name + f"  grid=({r['Grid_Size_X']},{r['Grid_Size_Y']},{r['Grid_Size_Z']})"
    grid[k][0] += 1; grid[k][1] += t
    tot += t
for agg, suffix in ((per, "kernel_stats.txt"), (grid, "kernel_stats_by_grid.txt")):
    with open(out + "_" + suffix, "w") as fh:
        fh.write("# " + header + "\n")
        fh.write(f"{'kernel':<135} {'calls':>7} {'total_ms':>10} {'avg_us':>10} {'pct':>6}\n")
        for k, (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:60]:
            fh.write(f"{k:<135} {n:>7} {t / 1e6:>10.3f} {t / n / 1e3:>10.2f} {100.0 * t / tot:>6.2f}\n")
        fh.write(f"TOTAL kernel time {tot / 1e6:.3f} ms\n")
PY
}
trace() {  # trace <tag> <header> <command ...>
  tag=$1; hdr=$2; shift 2
  (cd /tmp; export TMPDIR=/tmp; timeout 500 rocprofv3 --kernel-trace --stats -d $O/t_$tag -o p --output-format csv -- "$@" > $O/t_$tag.log 2>&1)
  summ $O/t_$tag $O/r04_final_$tag "$hdr"; rm -rf $O/t_$tag
}
# ---- headline: PMC traffic + MFMA utilisation, then the bench line, then the eager kernel trace
if want headline; then
bash scripts/pmc_families.sh step python bench.py --full --no-graph --steps 2 --warmup 1 --no-cpu-baseline --profile-steps 1 > $O/pmc_step.log 2>&1
cp gpurun_out/pmc_step/traffic.json profiles/r04_pmc_step_traffic.json; cp gpurun_out/pmc_step/traffic.json $O/r04_pmc_step_traffic.json
bash scripts/pmc_mfma.sh > $O/pmc_mfma.log 2>&1; cp gpurun_out/pmc_mfma/mfma_util.txt $O/r04_mfma_util.txt
timeout 600 python bench.py --full > $O/r04_final_bench.json 2> $O/bench.err
HC_FORCE_DIST=1 timeout 300 python bench.py --full --no-cpu-baseline > $O/r04_final_bench_forced_dist.json 2> $O/bench_dist.err
trace headline "rocprofv3 --kernel-trace --stats -- python bench.py --full --steps 12 --warmup 3 --no-graph --no-cpu-baseline --profile-steps 1  (MI355X; eager steps incl. warm-up + one instrumented step)" python $R/bench.py --full --steps 12 --warmup 3 --no-graph --no-cpu-baseline --profile-steps 1
timeout 120 python scripts/bench_ew.py 2>&1 | grep -v amdgpu > $O/r04_final_bn_passes.txt
timeout 200 python scripts/bench_s2.py 2>&1 | grep -v amdgpu > $O/r04_final_conv_s2_shapes.txt
timeout 120 python scripts/check_rows.py 2>&1 | grep -v amdgpu > $O/r04_final_conv_rows_shapes.txt
timeout 200 python scripts/bench_wrep.py 2>&1 | grep -v amdgpu > $O/r04_final_wgrad_rep_shapes.txt
fi
# ---- secondary configurations: PMC traffic, bench line (graph replay), eager trace
if want rexnet; then
bash scripts/pmc_families.sh rexnet python scripts/bench_rexnet.py --steps 2 --warmup 1 --no-graph --no-cpu-baseline > $O/pmc_rexnet.log 2>&1
cp gpurun_out/pmc_rexnet/traffic.json profiles/r04_pmc_rexnet_traffic.json; cp gpurun_out/pmc_rexnet/traffic.json $O/r04_pmc_rexnet_traffic.json
timeout 400 python scripts/bench_rexnet.py --steps 20 --warmup 5 > $O/r04_final_rexnet_bench.json 2> $O/rexnet.err
trace rexnet "rocprofv3 --kernel-trace --stats -- python scripts/bench_rexnet.py --steps 3 --warmup 1 --no-graph --no-cpu-baseline  (MI355X)" python $R/scripts/bench_rexnet.py --steps 3 --warmup 1 --no-graph --no-cpu-baseline
timeout 300 python scripts/bench_dw.py 2>&1 | grep -v amdgpu > $O/r04_final_dw_tile_shapes.txt
fi
if want yolov4; then
bash scripts/pmc_families.sh yolov4 python scripts/bench_yolov4.py --batch 16 --steps 2 --warmup 1 --no-graph --no-cpu-baseline > $O/pmc_yolov4.log 2>&1
cp gpurun_out/pmc_yolov4/traffic.json profiles/r04_pmc_yolov4_traffic.json; cp gpurun_out/pmc_yolov4/traffic.json $O/r04_pmc_yolov4_traffic.json
timeout 500 python scripts/bench_yolov4.py --batch 16 --steps 10 --warmup 3 > $O/r04_final_yolov4_bench.json 2> $O/yolov4.err
timeout 500 python scripts/bench_yolov4.py --eval --batch 16 --steps 10 --warmup 3 > $O/r04_final_yolov4_eval_bench.json 2> $O/yolov4_eval.err
timeout 300 python scripts/bench_bigtile.py 2>&1 | grep -v amdgpu > $O/r04_final_bigtile_family_shapes.txt
trace yolov4 "rocprofv3 --kernel-trace --stats -- python scripts/bench_yolov4.py --batch 16 --steps 3 --warmup 1 --no-graph --no-cpu-baseline  (MI355X)" python $R/scripts/bench_yolov4.py --batch 16 --steps 3 --warmup 1 --no-graph --no-cpu-baseline
fi
if want fp8; then
bash scripts/pmc_families.sh repvgg_a2_fp8 python scripts/bench_repvgg_fp8.py --steps 2 --warmup 1 > $O/pmc_fp8.log 2>&1
cp gpurun_out/pmc_repvgg_a2_fp8/traffic.json profiles/r04_pmc_repvgg_a2_fp8_traffic.json; cp gpurun_out/pmc_repvgg_a2_fp8/traffic.json $O/r04_pmc_repvgg_a2_fp8_traffic.json
timeout 300 python scripts/bench_repvgg_fp8.py > $O/r04_final_repvgg_a2_fp8_bench.json 2> $O/fp8.err
fi
if want mobileone; then
timeout 300 python scripts/bench_mobileone.py > $O/r04_final_mobileone_bench.json 2> $O/mobileone.err
fi
if want misc; then
ls -la $O | head -60
cut -c1-300 $O/r04_final_bench.json
timeout 200 python scripts/fixture_fracs.py 2>&1 | grep -v amdgpu > $O/fixture_fracs.txt; tail -1 $O/fixture_fracs.txt
timeout 400 python -m pytest tests/test_gpu_yolo.py -q -x 2>&1 | tail -5 > $O/yolo_tests.log; cat $O/yolo_tests.log
fi
