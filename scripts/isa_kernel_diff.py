#!/usr/bin/env python3
"""Two AMDGPU .s listings of the library (hipcc -S --cuda-device-only), kernel by kernel: which kernels' instruction sequences differ
(block labels normalised), and a census of named kernels.
usage: isa_kernel_diff.py parent.s change.s [kernel-name-substring ...]"""
import collections
import re
import sys


def kernels(path):
    out, cur, name = {}, None, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", ln)
        if m and not ln.startswith(".L"):
            name, cur = m.group(1), []
            continue
        if ln.startswith(".Lfunc_end"):
            if name is not None:
                out[name] = cur
            name = cur = None
            continue
        if cur is None:
            continue
        s = ln.split(";")[0].strip()
        if not s or s.startswith(".") and not s.startswith(".LBB"):
            continue
        cur.append(s)
    return out


def normalised(body):
    labels = {}
    for s in body:
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = "L%d" % len(labels)
    return [re.sub(r"\.LBB\d+_\d+", lambda m: labels.get(m.group(0), m.group(0)), s) for s in body]


def census(body):
    c = collections.Counter()
    for s in body:
        if s.endswith(":"):
            continue
        op = s.split()[0]
        c[op] += 1
    valu = sum(n for op, n in c.items() if op.startswith("v_"))
    ds = sum(n for op, n in c.items() if op.startswith("ds_"))
    vmem = sum(n for op, n in c.items() if op.startswith(("global_", "buffer_", "flat_", "scratch_")))
    skip = ("s_waitcnt", "s_nop", "s_cbranch", "s_branch", "s_load", "s_buffer_load", "s_barrier", "s_endpgm", "s_sched")
    salu = sum(n for op, n in c.items() if op.startswith("s_") and not op.startswith(skip))
    return c, {"VALU": valu, "DS": ds, "VMEM": vmem, "SALU": salu, "all": sum(c.values())}


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
same = [k for k in a if k in b and normalised(a[k]) == normalised(b[k])]
diff = [k for k in a if k in b and k not in same]
print("kernels: parent %d, change %d; identical %d; different %d: %s" % (len(a), len(b), len(same), len(diff), diff))
print("only in parent:", [k for k in a if k not in b])
print("only in change:", [k for k in b if k not in a])
for pat in sys.argv[3:]:
    for side, ks in (("parent", a), ("change", b)):
        for k in ks:
            if pat in k:
                c, tot = census(ks[k])
                print(side, k, tot)
                print("   ", sorted(c.items(), key=lambda kv: -kv[1])[:40])
