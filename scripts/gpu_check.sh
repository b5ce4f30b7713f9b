#!/bin/bash
# One call on a machine with an MI355X: GPU parity tests, smoke, the full bench line (+variants), rocprofv3 kernel trace + PMC passes of the headline leg.
# usage: bash scripts/gpu_check.sh <output directory>
OUT=${1:?usage: bash scripts/gpu_check.sh <output directory>}
mkdir -p $OUT; rm -rf $OUT/prof $OUT/pmc*
OUT=$(cd $OUT && pwd)
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
echo "== pytest gpu"; timeout 900 python -m pytest tests -x -q -m gpu 2>&1 | tail -8 | tee $OUT/pytest_gpu.log
echo "== smoke"; timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2 | tee $OUT/smoke.log
echo "== bench"; timeout 600 python bench.py --full 2>&1 | tail -1 | tee $OUT/bench.json
echo "== bench, the N > 1 code path on this one GPU (two ranks on cuda:0, gloo for the collectives: sharding / max over ranks / per-rank rates run; the numbers mean nothing)"
RBD_BENCH_ONE_DEVICE=1 timeout 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 10 --warmup 3 2>/dev/null | tail -1 | cut -c1-400 | tee $OUT/bench_two_ranks.json
echo "== bench variants"; rm -f $OUT/bench_variants.jsonl
for extra in "--graph" "--dtype f32" "--dtype f32 --batch 65536 --steps 200" "--batch 65536 --steps 200" "--layout soa" "--wrenches" "--model atlas_fixed" "--batch 524288 --steps 30 --dtype f32"; do
  timeout 600 python bench.py --full --no-cpu-baseline $extra 2>&1 | tail -1 >> $OUT/bench_variants.jsonl
done
python - $OUT/bench_variants.jsonl <<'PY'
import json, sys
for l in open(sys.argv[1]):
    try:
        d = json.loads(l); c = d["config"]
        print(f"{c['workload'][:60]:60s} graph={c['hip_graph']} layout={c['layout']} wrenches={c['external_wrenches']}: {d['value']/1e6:8.1f} Mevals/s kernel {d['roofline']['kernel_ms']*1e3:8.2f} us err {d['parity_rel_err_vs_oracle']:.1e}")
    except Exception as e:
        print("bad line", l[:200])
PY
echo "== rocprof kernel trace"
cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python $R/bench.py --steps 500 > $OUT/rocprof_run.log 2>&1
rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS --output-format csv -d $OUT/pmc1 -- python $R/bench.py --steps 100 --warmup 10 > /dev/null 2>&1
rocprofv3 --pmc SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT --output-format csv -d $OUT/pmc2 -- python $R/bench.py --steps 100 --warmup 10 > /dev/null 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc3 -- python $R/bench.py --steps 100 --warmup 10 > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc4 -- python $R/bench.py --steps 100 --warmup 10 > /dev/null 2>&1
cd $R
python scripts/summarize_prof.py $OUT | tee $OUT/prof_summary.txt
