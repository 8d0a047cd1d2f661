#!/bin/bash
# the measurements committed under profiles/r04_* (one gpurun call): kernel trace + PMC passes of bench.py, the authors' schedule through
# the driver (incremental post-filter chain), its per-kernel profile, the 2-rank rehearsal of bench.py, and bench.py itself
R=$PWD
O=out/r04final
mkdir -p $O
tools/prof_bench.sh r04final/prof > $O/prof_bench.log 2>&1
python3 tools/authors_schedule.py 64 > $O/authors_schedule_64x1080p.txt 2>&1
tools/prof_postfilter.sh r04final/pf 16 > $O/postfilter_profile.txt 2>&1
HCMVS_BENCH_ONE_DEVICE=1 HCMVS_BENCH_BACKEND=gloo python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 1 --warmup 0 --batch 4 --no-pmc > $O/bench_2rank_rehearsal.json 2> $O/bench_2rank_rehearsal.err
python3 bench.py --full > $O/bench.json 2> $O/bench.err
tail -c 2500 $O/bench.json
echo; tail -c 600 $O/bench_2rank_rehearsal.json
