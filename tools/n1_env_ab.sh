# A/B of finalize variants at 1B rows: bash tools/n1_env_ab.sh "label:ENV=1" "label2:" (on a machine with an MI355X).
# Each variant: rocprofv3 kernel stats over one warm n1 step -> $OUT/n1env_<label>/ (default run_out/).
cd /tmp && export TMPDIR=/tmp; cd "$(dirname "$(readlink -f "$0")")/.." || exit 1
OUT=${OUT:-run_out}
mkdir -p "$OUT"
for spec in "$@"; do
  label=${spec%%:*}; envs=${spec#*:}
  env $envs timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $OUT/n1env_$label -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-engine-leg --no-n1-parity --no-pmc --rows-per-gpu 1000000 > $OUT/n1env_$label.log 2>&1 || exit 1
done
