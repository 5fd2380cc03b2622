"""Post-process a rocprofv3 --kernel-trace CSV of bench.py: per iteration, the critic-step window from the first
k_build_critic_input* after the previous generator Adam to the critic Adam of that iteration's last critic step; the
whole iteration; and, per queue, busy time inside the window (overlap check).  Also dumps one iteration's dispatches.
usage: trace_window.py TRACE_DIR N_CRITIC OUT_PREFIX"""
import csv, glob, re, sys, collections

tdir, ncrit, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
f = glob.glob(tdir + "/**/*kernel_trace.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
qkey = "Queue_Id" if "Queue_Id" in rows[0] else None
skey = "Stream_Id" if "Stream_Id" in rows[0] else None
nm = lambda r: re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").strip()
S = lambda r: int(r["Start_Timestamp"])
E = lambda r: int(r["End_Timestamp"])
adam = [i for i, r in enumerate(rows) if nm(r).startswith("k_adam")]
per_it = ncrit + 1
# iterations = groups of ncrit + 1 Adams; keep the last 4 full ones
its = [adam[k:k + per_it] for k in range(len(adam) % per_it, len(adam), per_it)][-4:]
lines = []
for it in its:
    prev_g = it[0] - 1
    while prev_g >= 0 and not nm(rows[prev_g]).startswith("k_adam"):
        prev_g -= 1
    lo = prev_g + 1
    # last critic step: starts after the (ncrit-1)-th critic Adam of this iteration
    c_lo = it[ncrit - 2] + 1 if ncrit > 1 else lo
    bci = next(i for i in range(c_lo, it[ncrit - 1]) if nm(rows[i]).startswith("k_build_critic_input"))
    cad = it[ncrit - 1]
    t0, t1 = S(rows[bci]), E(rows[cad])
    inwin = [r for r in rows[lo:it[-1] + 1] if S(r) < t1 and E(r) > t0]
    busy = collections.defaultdict(int)
    for r in inwin:
        busy[r.get(qkey, "?") if qkey else "?"] += min(E(r), t1) - max(S(r), t0)
    it_wall = E(rows[it[-1]]) - E(rows[prev_g]) if prev_g >= 0 else 0
    lines.append(f"iteration: wall {it_wall / 1e6:.3f} ms (gen Adam to gen Adam); critic window "
                 f"k_build_critic_input -> critic k_adam {(t1 - t0) / 1e6:.3f} ms, {len(inwin)} dispatches; "
                 "busy per queue in the window: " + ", ".join(f"q{q} {b / 1e6:.3f} ms" for q, b in sorted(busy.items())))
# one iteration's dispatches (the last) with queue, start offset and duration
it = its[-1]
prev_g = it[0] - 1
while not nm(rows[prev_g]).startswith("k_adam"):
    prev_g -= 1
t0 = E(rows[prev_g])
with open(out + "_dispatch.txt", "w") as fo:
    fo.write("# start_us  dur_us  queue stream  workgroups  kernel (one iteration, sorted by start; t = 0 at the previous generator Adam's end)\n")
    for r in rows[prev_g + 1:it[-1] + 1]:
        wg = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
        fo.write(f"{(S(r) - t0) / 1e3:9.1f} {(E(r) - S(r)) / 1e3:8.1f}  q{r.get(qkey, '?') if qkey else '?':>3} "
                 f"s{r.get(skey, '?') if skey else '?':>3} {wg:7d}  {nm(r)[:110]}\n")
with open(out + "_window.txt", "w") as fo:
    fo.write("\n".join(lines) + "\n")
print("\n".join(lines))
