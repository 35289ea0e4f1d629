"""Compare two cross-compiles of the generation translation units, kernel by kernel.

Each directory holds, per unit U of gen_mlp / mlp / gen_rows / generate,
    U.s      hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S U.hip
    U.rpass  that command's -Rpass-analysis=kernel-resource-usage remarks (stderr)

    python tools/gen_build_compare.py OLD_DIR NEW_DIR

prints, for every kernel of OLD_DIR, whether NEW_DIR's resource columns (VGPR / AGPR / SGPR /
scratch / waves per SIMD / spills / LDS) and device ISA are identical (the ISA is the kernel's
instructions, labels and kernel descriptor fields; comments, other directives, the function
ordinal in local labels and the descriptor's kernarg size dropped),
then every kernel only NEW_DIR has, beside its twin (the same mangled name with the last
template digit one lower, where OLD or NEW has it).  Exit status 1 if an old kernel differs.
No GPU is needed.
"""
import os
import re
import subprocess
import sys

UNITS = ('gen_mlp', 'mlp', 'gen_rows', 'generate')
COLS = ('VGPRs', 'AGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]',
        'SGPRs Spill', 'VGPRs Spill', 'LDS Size [bytes/block]')


def resources(path):
    out, cur = {}, None
    for line in open(path, errors='replace'):
        m = re.search(r'remark:\s+(.*?) \[-Rpass-analysis', line)
        if not m:
            continue
        k, _, v = m.group(1).partition(': ')
        if k == 'Function Name':
            cur = out.setdefault(v.strip(), {})
        elif cur is not None:
            cur[k.strip()] = v.strip()
    return out


def bodies(path):
    """{kernel symbol: its instruction lines}"""
    out, cur, name = {}, None, None
    for line in open(path, errors='replace'):
        m = re.match(r'^(_Z\w+):', line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = cur
            cur = None
            continue
        t = line.split(';')[0].strip()
        # (instructions and labels; of the directives only the kernel descriptor's fields, less
        #  the size of the argument block, which grows with GenMlpArgs and moves no offset)
        if not t or (t.startswith('.') and not t.endswith(':') and
                     not t.startswith('.amdhsa_')) or t.startswith('.amdhsa_kernarg_size'):
            continue
        # (local labels carry the function's ordinal in its module)
        cur.append(re.sub(r'\.L(BB|JTI|tmp|func_begin|func_end)\d+', r'.L\1N', t))
    return out


def demangle(names):
    try:
        r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True)
        return dict(zip(names, r.stdout.split('\n')))
    except OSError:
        return {n: n for n in names}


def row(r):
    return ' / '.join(r.get(c, '?') for c in COLS)


def main(old, new):
    bad = 0
    print('columns: ' + ' / '.join(COLS))
    for u in UNITS:
        ro, rn = resources(os.path.join(old, u + '.rpass')), resources(os.path.join(new, u + '.rpass'))
        bo, bn = bodies(os.path.join(old, u + '.s')), bodies(os.path.join(new, u + '.s'))
        dm = demangle(sorted(set(ro) | set(rn)))
        print('== %s.hip: %d kernels before, %d after' % (u, len(ro), len(rn)))
        for k in sorted(ro):
            same_r = k in rn and all(ro[k].get(c) == rn[k].get(c) for c in COLS)
            same_i = k in bn and bo.get(k) == bn.get(k)
            if not (same_r and same_i):
                bad += 1
                print('  DIFFERS %s\n      old %s\n      new %s  (ISA %s)'
                      % (dm[k], row(ro[k]), row(rn.get(k, {})), 'same' if same_i else 'differs'))
        print('  old kernels identical in every column and in ISA: %d of %d'
              % (sum(1 for k in ro if k in rn and all(ro[k].get(c) == rn[k].get(c) for c in COLS)
                     and bo.get(k) == bn.get(k)), len(ro)))
        for k in sorted(set(rn) - set(ro)):
            print('  new  %s\n      %s   (%d instructions)' % (dm[k], row(rn[k]), len(bn.get(k, []))))
            # the twin: the last 'Li3E' of the mangled name one level lower
            # (the per-sample scored kernels are not template builds: X_scored_kernel's twin is
            #  X_kernel<2>)
            i = k.rfind('Li3E')
            tw = k[:i] + 'Li2E' + k[i + 4:] if i >= 0 else None
            if tw is None and '_scored_kernel' in dm[k]:
                want = dm[k].split('(')[0].replace('_scored_kernel', '_kernel<2>')
                tw = next((t for t in rn if dm[t].startswith('void ' + want + '(')), None)
            if tw in rn:
                print('      twin %s   (%d instructions)' % (row(rn[tw]), len(bn.get(tw, []))))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
