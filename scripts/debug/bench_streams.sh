for s in 2 3 2 3 4; do python bench.py --steps 20 --warmup 5 --streams $s --full --no-extras --no-cpu-baseline 2>/dev/null | tail -1 | python -c '
import json, sys
d = json.loads(sys.stdin.read()); r = d["roofline"]
print("streams tried", d["config"]["streams_tried"], "used", d["config"]["streams"], "multi", r["regions_us_multi_stream"], "one", r["regions_us_one_stream"])
'
done
