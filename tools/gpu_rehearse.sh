# 2-rank rehearsal of the multi-GPU bench path on one GPU (gloo, real HIP kernels).
#     bash tools/gpu_rehearse.sh [tag] [output directory]
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp TW_BENCH_BACKEND=gloo
O=${2:-bench_out}
mkdir -p "$O"
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 5 --warmup 2 --no-sgd > "$O/${1:-r1}_rehearse2.json" 2> "$O/${1:-r1}_rehearse2.err"
