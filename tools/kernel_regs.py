"""Device code of two builds of the library, side by side: per kernel the VGPR and SGPR counts, scratch and LDS bytes, and the
instruction text (a kernel under a tight register cap can tip into scratch on a harmless-looking change: round 6, k_x1 12 -> 104
bytes; a kernel that moves to another translation unit must come out the same).  Compile every unit of both builds with
hipcc ... --save-temps, then
    python tools/kernel_regs.py <new> <old>            # each side: directories and / or *gfx950.s files, comma-separated
Over all units of a side: the set of kernel names must agree (none missing, none new, none twice), and every kernel's resources and
instructions -- labels and comments stripped -- must be equal.  Prints what differs and exits 1 if anything does."""
import collections, glob, hashlib, os, re, subprocess, sys

FIELDS = ('next_free_vgpr', 'next_free_sgpr', 'private_segment_fixed_size', 'group_segment_fixed_size')


def files(side):
    out = []
    for p in side.split(','):
        out += sorted(glob.glob(os.path.join(p, '**', '*gfx950.s'), recursive=True)) if os.path.isdir(p) else [p]
    return out


def body(txt, name):
    """Instruction text of one function: from its label to its .Lfunc_end, without directives (the kernel descriptor among
    them), labels, comments and blank lines."""
    m = re.search(r'^' + re.escape(name) + r':[^\n]*\n(.*?)^\.Lfunc_end\d+:', txt, re.S | re.M)
    lines = []
    for line in m.group(1).split('\n'):
        line = re.sub(r'\s*;.*$', '', line).strip()
        if not line or line.startswith('.'):
            continue
        lines.append(re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', line))   # the function's number within its unit is not part of the code
    return lines


def parse(paths):
    out, twice = {}, []
    for p in paths:
        txt = open(p).read()
        for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, re.S):
            name, desc = m.group(1), m.group(2)
            res = tuple(int(re.search(r'\.amdhsa_%s (\d+)' % f, desc).group(1)) for f in FIELDS)
            ins = body(txt, name)
            if name in out:
                twice.append(name)
            out[name] = (res, len(ins), hashlib.sha1('\n'.join(ins).encode()).hexdigest(), os.path.basename(p))
    return out, twice


def dem(n):
    try:
        return subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()[:100]
    except Exception:
        return n[:100]


if __name__ == '__main__':
    (new, twice_new), (old, twice_old) = parse(files(sys.argv[1])), parse(files(sys.argv[2]))
    bad = 0
    for what, names in (('only in new', set(new) - set(old)), ('only in old', set(old) - set(new)), ('twice in new', twice_new), ('twice in old', twice_old)):
        for k in sorted(names):
            print(f'{what}: {dem(k)}')
            bad += 1
    for k in sorted(set(new) & set(old)):
        if new[k][0] != old[k][0]:
            print(f'resources differ (vgpr, sgpr, scratch, lds): {dem(k)}  old {old[k][0]} [{old[k][3]}]  new {new[k][0]} [{new[k][3]}]')
            bad += 1
        elif new[k][2] != old[k][2]:
            print(f'instructions differ: {dem(k)}  old {old[k][1]} [{old[k][3]}]  new {new[k][1]} [{new[k][3]}]')
            bad += 1
    units = lambda d: dict(collections.Counter(v[3] for v in d.values()))
    print(f'{len(new)} kernels in new {units(new)}, {len(old)} in old {units(old)}: {bad} differences')
    sys.exit(1 if bad else 0)
