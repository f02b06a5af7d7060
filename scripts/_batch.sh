cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
out=${1:?usage: scripts/_batch.sh OUTDIR}
mkdir -p $out
timeout 1800 python -m pytest tests/test_gpu_kernels.py tests/test_gpu_solvers.py tests/test_gpu_fullsize.py tests/test_gpu_dist2.py -x -q -m gpu -k "lu or solve or iar or refine or factor or beyn or nleigs or c3 or c4 or plan or thread or dist or rank" > $out/pytest.log 2>&1
python bench.py --steps 30 --warmup 5 --full --no-c5 --no-cold > $out/bench_g1.json 2> $out/bench.err
NEP_LU_GRAPH=0 python bench.py --steps 30 --warmup 5 --full --no-c5 --no-cold > $out/bench_g0.json 2>> $out/bench.err
python bench.py --steps 30 --warmup 5 --full --no-c5 --no-cold > $out/bench_g1b.json 2>> $out/bench.err
