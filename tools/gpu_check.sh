set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${OUT:-out}/fin
mkdir -p $O
timeout -k 10 900 python -m pytest tests -q -x -m gpu > $O/gpu_tests.log 2>&1
tail -3 $O/gpu_tests.log
python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
tail -2 $O/smoke.log
python bench.py --full > $O/bench.json 2> $O/bench.err
tail -c 3000 $O/bench.json
