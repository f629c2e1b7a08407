"""Instruction identity of the kernels of two ISA dumps (scripts/isa.sh):  python scripts/isa_diff.py before.s after.s
                    ... of the per-group-size copies of one dump:           python scripts/isa_diff.py --copies dump.s
A kernel's text is what stands between its label and its .Lfunc_end; comments, symbol names and the function number in local labels are
stripped, every instruction and label is kept. Register figures that match are not enough: the scheduler's occupancy target follows
the flat work-group size and can reorder instructions without moving a register count.
Kernels are matched by name. A k_extend of `after` without a group size among its template arguments (<MODE, FEAT, COUNT, DRAIN, LIST>) is
compared with the copy of `before` that was compiled for the largest group (<MODE, FEAT, COUNT, TPB, DRAIN, LIST>); one with a seventh
argument `false` (<..., LIST, ANYHIT = false>) with the six-argument instance of `before`."""
import re, subprocess, sys


def kernels(path):
    """demangled name (without arguments) -> list of instruction lines"""
    text = open(path).read()
    names = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M)
    dem = subprocess.run(['c++filt'], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, dem):
        body = text[text.index(f"\n{n}:") + 1:]
        body = body[:re.search(r'^\.Lfunc_end\d+:', body, re.M).start()]
        lines = []
        for ln in body.split("\n")[1:]:
            ln = re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0]).replace(n, 'SELF').strip()
            if ln:
                lines.append(ln)
        out[re.sub(r'^void ', '', re.sub(r'\(.*', '', d.replace('(anonymous namespace)', '{anonymous}')))] = lines   # (denoise.hip's kernels)
    return out


def split_tpb(name):
    """('k_extend<M, F, C, D, L>', TPB) for a k_extend with six template arguments, else (name, None)"""
    m = re.fullmatch(r'(rtk::k_extend<)(.*)>', name)
    a = m.group(2).split(', ') if m else []
    if len(a) != 6:
        return name, None
    return m.group(1) + ', '.join(a[:3] + a[4:]) + '>', int(a[3].rstrip('u'))


def merged(ks):
    """kernels under their names without a group size: name -> {TPB or None: lines}"""
    out = {}
    for n, lines in ks.items():
        key, tpb = split_tpb(n)
        out.setdefault(key, {})[tpb] = lines
    return out


if sys.argv[1] == '--copies':
    same = diff = 0
    for key, copies in sorted(merged(kernels(sys.argv[2])).items()):
        if len(copies) < 2:
            continue
        ref = copies[max(copies)]
        for tpb in sorted(copies)[:-1]:
            if copies[tpb] == ref:
                same += 1
            else:
                diff += 1
                print(f"DIFFERS {key}: {tpb} threads {len(copies[tpb])} lines, {max(copies)} threads {len(ref)} lines")
    print(f"{same + diff} smaller-group copies compared with their largest-group copy: {same} identical, {diff} differ")
else:
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    # a k_extend of `after` with a seventh template argument `false` (ANYHIT, defaulted: added after `before` was taken) is the instance
    # `before` lists with six
    # (only where `before` does not list the seven-argument name itself: two dumps taken after ANYHIT was added match by name)
    b = {(n[:-len(', false>')] + '>' if n not in a and re.fullmatch(r'rtk::k_extend<([^,]*, ){6}false>', n) else n): v for n, v in b.items()}
    by_key = merged(a)
    same = diff = 0
    used = set()
    for name in sorted(b):
        if name in a:
            ref, src = a[name], name
        elif name in by_key:        # a k_extend that lost its group size: against the copy for the largest group
            tpb = max(by_key[name])
            ref = by_key[name][tpb]
            src = next(n for n in a if split_tpb(n) == (name, tpb))
        else:
            print("ONLY IN", sys.argv[2], name)
            continue
        used.add(src)
        if ref == b[name]:
            same += 1
        else:
            diff += 1
            print(f"DIFFERS {name}: {len(ref)} -> {len(b[name])} lines")
    for name in sorted(set(a) - used):
        print("ONLY IN", sys.argv[1], name)
    print(f"{len(a)} kernels before, {len(b)} after; {same + diff} compared: {same} identical, {diff} differ; {len(a) - len(used)} only before")
