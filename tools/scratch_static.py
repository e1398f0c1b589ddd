"""Static scratch traffic of the functions of a gfx950 assembly file (hipcc -S --cuda-device-only).

    python tools/scratch_static.py FILE.s [NAME-SUBSTRING ...]
Per function whose demangled name contains one of the substrings (default: k_ipm, loop_ipm, k_qp):
scratch dword stores / loads in the body; those inside the widest loop that holds calls (the IPM's
iteration loop); and those inside call-free loops (the lane loops of the inlined passes).  A loop is
the span of a backward branch: its label .. the branch.  Counts are of instructions weighted by their
width in dwords; nothing is run."""
import re
import subprocess
import sys

WIDTH = {"dword": 1, "dwordx2": 2, "dwordx3": 3, "dwordx4": 4, "b32": 1, "b64": 2, "b96": 3, "b128": 4}


def functions(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            if name:
                yield name, body
            name, body = m.group(1), []
        elif name:
            if line.startswith(".Lfunc_end"):
                yield name, body
                name, body = None, []
            else:
                body.append(line)
    if name:
        yield name, body


def count(lines):
    st = ld = 0
    for ln in lines:
        m = re.match(r"\s*scratch_(load|store)_(\w+)", ln)
        if m:
            w = WIDTH.get(m.group(2), 1)
            if m.group(1) == "load":
                ld += w
            else:
                st += w
    return st, ld


def analyse(body):
    labels = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", ln)] if m}
    loops = []
    for j, ln in enumerate(body):
        m = re.match(r"\s*s_c?branch\w*\s+(\.LBB\w+)", ln)
        if m and labels.get(m.group(1), j + 1) <= j:
            loops.append((labels[m.group(1)], j))
    calls = [i for i, ln in enumerate(body) if "s_swappc_b64" in ln]
    with_calls = [(a, b) for a, b in loops if any(a <= c <= b for c in calls)]
    lane = [(a, b) for a, b in loops if not any(a <= c <= b for c in calls)]
    in_lane = set()
    for a, b in lane:
        in_lane.update(range(a, b + 1))
    it = max(with_calls, key=lambda r: r[1] - r[0]) if with_calls else None
    return dict(body=count(body), iteration=count(body[it[0]:it[1] + 1]) if it else (0, 0),
                lane=count([body[i] for i in sorted(in_lane)]),
                lane_in_iteration=count([body[i] for i in sorted(in_lane) if it and it[0] <= i <= it[1]]),
                calls_in_iteration=sum(1 for c in calls if it and it[0] <= c <= it[1]))


if __name__ == "__main__":
    want = sys.argv[2:] or ["k_ipm", "loop_ipm", "k_qp"]
    fs = list(functions(sys.argv[1]))
    dem = subprocess.run(["c++filt"], input="\n".join(n for n, _ in fs), capture_output=True, text=True).stdout.split("\n")
    print("%-78s %13s %13s %13s %13s %5s" % ("function (stores / loads, dwords)", "body", "iter. loop", "lane loops", "lane in iter.", "calls"))
    for (n, body), d in zip(fs, dem):
        short = re.sub(r"\(.*", "", d)
        if not any(w in short.split("<")[0] for w in want):
            continue
        r = analyse(body)
        print("%-78s %13s %13s %13s %13s %5d" % (short[-78:], *("%d / %d" % r[k] for k in ("body", "iteration", "lane", "lane_in_iteration")),
                                                 r["calls_in_iteration"]))
