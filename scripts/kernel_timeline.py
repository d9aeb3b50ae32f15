"""Start / end / duration per kernel and queue out of a `rocprofv3 --kernel-trace --output-format csv` directory:
python scripts/kernel_timeline.py TRACE_DIR [ROWS] > timeline.txt   (the last ROWS launches of the level-1 step's kernels, default 80)"""
import csv, glob, os, sys

KEYS = ("k_l1_", "k_scan", "k_decode", "k_parse_gate", "k_rec_verify")


def main():
    d = sys.argv[1]
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 80
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows = [r for r in rows if any(k in r["Kernel_Name"] for k in KEYS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if not rows:
        print("no kernels found under", d, file=sys.stderr)
        return 1
    t0 = int(rows[0]["Start_Timestamp"])
    for r in rows[-last:]:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:30]
        print("%-30s q%-3s start %10.3f ms  end %10.3f ms  dur %9.3f" % (name, r.get("Queue_Id", "?"), (s - t0) / 1e6, (e - t0) / 1e6, (e - s) / 1e6))
    return 0


if __name__ == "__main__":
    sys.exit(main())
