"""Audits the gfx950 ISA of libmpcombi_hip for the VGPR index mode the register simplex relies on (lp_reg.hpp: a tableau
column chosen at run time is read / written through s_set_gpr_idx_on ... s_set_gpr_idx_off).  While the mode is on EVERY
vector instruction is index-shifted, so a region must be short, closed, and free of control flow.  (During development a
build with an early `return` between an indexed read and an indexed write produced wrong verdicts and memory faults; the
source was restructured, and this check makes the property visible.)

    python tools/check_gpr_idx.py [file.s]      # without an argument: compiles every unit of the library with --save-temps
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def audit(text: str):
    on, bad, total, longest, func = None, [], 0, 0, None
    for i, line in enumerate(text.split('\n')):
        t = line.strip()
        if re.match(r'^_ZN3mpc\w+:', line):
            func = line.split(':')[0]
        if t.startswith('s_set_gpr_idx_on'):
            if on is not None:
                bad.append((func, i, 'nested s_set_gpr_idx_on'))
            on, total = i, total + 1
        elif t.startswith('s_set_gpr_idx_off'):
            if on is None:
                bad.append((func, i, 's_set_gpr_idx_off without on'))
            else:
                longest = max(longest, i - on)
            on = None
        elif on is not None and re.match(r'^(s_cbranch|s_branch|s_endpgm|s_setpc|s_swappc|\.LBB)', t):
            bad.append((func, i, 'control flow inside an index-mode region: ' + t))
    if on is not None:
        bad.append((func, on, 'index mode left on'))
    return total, longest, bad


def assembly() -> str:
    """The gfx950 assembly of every translation unit of the library (the list and the flags of __graft_entry__.py, so that a unit
    which starts to use the index mode cannot be missed), compiled side by side and concatenated."""
    sys.path.insert(0, ROOT)
    try:
        import __graft_entry__ as entry
    finally:
        sys.path.remove(ROOT)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for src, _ in entry.HIP_UNITS:
            d = os.path.join(tmp, os.path.splitext(src)[0])
            os.mkdir(d)
            jobs.append((d, subprocess.Popen([hipcc, *entry.HIPCC_FLAGS, '-c', os.path.join(entry.CSRC, src), '-o', os.path.join(d, 'x.o'), '--save-temps'],
                                             cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)))
        text = []
        for d, proc in jobs:
            if proc.wait() != 0:
                raise subprocess.CalledProcessError(proc.returncode, 'hipcc --save-temps in ' + d)
            text += [open(os.path.join(d, f)).read() for f in os.listdir(d) if f.endswith('gfx950.s')]
        return '\n'.join(text)


if __name__ == '__main__':
    text = open(sys.argv[1]).read() if len(sys.argv) > 1 else assembly()
    total, longest, bad = audit(text)
    print(f'{total} index-mode regions, longest {longest} lines, {len(bad)} malformed')
    for b in bad:
        print(' ', b)
    sys.exit(1 if bad or total == 0 else 0)
