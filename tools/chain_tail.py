"""The end of every leading-tail chain round in a rocprofv3 kernel trace: the round's closing kernel (k_readback behind
the round's extra k_pass_lead; or k_lead_close, the one-workgroup kernel in place of both that profiles/lead_close/AB.md
measured as an A/B library), the k_pass_lead dispatches ahead of it, the gap between them, and the chain's tail = end of
the last kernel that ran a body .. end of the closing kernel.
   tools/chain_tail.py run_kernel_trace.csv WARMUP_ROUNDS"""
import csv
import statistics
import sys

path, warm = sys.argv[1], int(sys.argv[2])
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path))))
rounds, lead = [], []
for s, e, name in rows:
    if "k_pass_lead" in name:
        lead.append((s, e))
    elif "k_lead_close" in name or "k_readback" in name:
        if lead:
            rounds.append((lead, (s, e), "k_lead_close" in name))
        lead = []
    elif "k_align_init" in name:
        lead = []
rounds = rounds[warm:]


def line(label, xs):
    xs = [x / 1e3 for x in xs]
    if xs:
        print(f"{label:58s} n {len(xs):6d}  mean {statistics.fmean(xs):7.2f}  median {statistics.median(xs):7.2f}  "
              f"min {min(xs):7.2f}  max {max(xs):7.2f} us")


closing = "k_lead_close" if rounds and rounds[0][2] else "k_readback"
print(f"{len(rounds)} rounds after {warm} warm-up rounds; closing kernel {closing}; "
      f"k_pass_lead dispatches per round {statistics.fmean(len(l) for l, _, _ in rounds):.2f}")
line("k_pass_lead, last dispatch of a round", [l[-1][1] - l[-1][0] for l, _, _ in rounds])
line("k_pass_lead, the others", [e - s for l, _, _ in rounds for s, e in l[:-1]])
line("k_pass_lead start to start, the others", [b[0] - a[0] for l, _, _ in rounds for a, b in zip(l[:-2], l[1:-1])])
line("k_pass_lead start to start, into the last dispatch", [l[-1][0] - l[-2][0] for l, _, _ in rounds if len(l) > 1])
line(closing, [c[1] - c[0] for _, c, _ in rounds])
line(f"gap: last k_pass_lead end .. {closing} start", [c[0] - l[-1][1] for l, c, _ in rounds])
# the last kernel that ran a body: the last k_pass_lead ahead of k_lead_close, the one before the last ahead of k_readback
line("tail: last body kernel's end .. closing kernel's end",
     [c[1] - (l[-1][1] if new else l[-2][1]) for l, c, new in rounds if new or len(l) > 1])
