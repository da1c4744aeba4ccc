cd "$(dirname "$0")/.."; export TMPDIR=/tmp; OUT=${1:-build/bench}; mkdir -p "$OUT"
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout 1800 python -m pytest tests -m gpu -x -q > "$OUT/r04_final_pytest.log" 2>&1; grep -v "^W2026\|^HIP ver\|^ROCm ver\|^Hostname\|^Librccl\|^RCCL" "$OUT/r04_final_pytest.log" | tail -6
python3 bench.py --full --late 300 --late-steps 20 > "$OUT/r04_c4_bench.json" 2>/tmp/b.err || tail -3 /tmp/b.err
OUT=$OUT python3 -c "
import json, os; o=json.load(open(os.path.join(os.environ['OUT'], 'r04_c4_bench.json'))); print(o['ms_per_step'], o['value'], o['roofline']['frac'], o['roofline']['traffic_source'], o['roofline_groups']['p2g_plus_pcg']['frac'])"
