#!/usr/bin/env python3
"""Resource table of every hmc_gauss_persist_kernel instantiation, parent -> branch:
  scripts/gauss_resources.py <parent tree> <branch tree> "<title>" [extra hipcc flags] > profiles/<name>.txt
Compiles hmc_gauss.hip, hmc_gauss_rng.hip and hmc_gauss_rng_wide.hip of both trees for the
device alone with -Rpass-analysis=kernel-resource-usage and prints, per instantiation, VGPRs,
SGPRs, scratch and occupancy of both; the last lines count what changed.  No GPU needed."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FILES = ['hmc_gauss.hip', 'hmc_gauss_rng.hip', 'hmc_gauss_rng_wide.hip']
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '--cuda-device-only',
         '-Rpass-analysis=kernel-resource-usage', '-c', '-o', os.devnull]


def template_args(mangled):
    """'16, true, true, false, 0, 0, true, 3' from the kernel's mangled name (Li16E Lb1E ... Lin1E)."""
    m = re.match(r'_ZN4binf24hmc_gauss_persist_kernelI((?:L[ib]n?\d+E)+)E', mangled)
    if not m:
        return None
    out = []
    for kind, val in re.findall(r'L([ib])(n?\d+)E', m.group(1)):
        out.append(('true' if val == '1' else 'false') if kind == 'b' else val.replace('n', '-'))
    return ', '.join(out)


def resources(tree, name, extra):
    err = subprocess.run([HIPCC] + FLAGS + extra + [os.path.join(tree, 'binf_amd', 'csrc', name)],
                         text=True, capture_output=True, check=True).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r'remark: .*?Function Name: (\S+)', line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        for key, tag in (('v', r' VGPRs: (\d+)'), ('s', r' TotalSGPRs: (\d+)'),
                         ('scr', r' ScratchSize \[bytes/lane\]: (\d+)'), ('occ', r' Occupancy \[waves/SIMD\]: (\d+)')):
            m = re.search(tag, line)
            if m and cur is not None:
                res[cur][key] = int(m.group(1))
    table = {}
    for k, v in res.items():
        name = template_args(k)
        if name is not None:
            table[name] = v
    return table


def main():
    parent, branch, title = sys.argv[1:4]
    extra = sys.argv[4:]
    jobs = [(t, f) for f in FILES for t in (parent, branch)]
    with ThreadPoolExecutor(max_workers=6) as ex:
        got = list(ex.map(lambda j: resources(j[0], j[1], extra if j[0] == branch else []), jobs))
    print('hmc_gauss_persist_kernel<TMAX, REGULAR, UNIT, FMA, LW, RNG, UDT, HC>: '
          '-Rpass-analysis=kernel-resource-usage, parent -> %s' % title)
    print('(every instantiation; v = VGPRs, s = SGPRs, scr = scratch bytes per lane, occ = waves per SIMD)')
    total = changed = lost = scratch = 0
    for i, f in enumerate(FILES):
        a, b = got[2 * i], got[2 * i + 1]
        print('\n== %s' % f)
        assert list(a) == list(b), 'the two trees instantiate different kernels in ' + f
        for k in a:
            x, y = a[k], b[k]
            total += 1
            changed += x != y
            lost += y['occ'] < x['occ']
            scratch += y['scr'] > x['scr']
            print('%-60s v %3d->%3d s %3d->%3d scr %d->%d occ %d->%d%s' % (
                k, x['v'], y['v'], x['s'], y['s'], x['scr'], y['scr'], x['occ'], y['occ'],
                '   *' if x != y else ''))
    print('\n%d instantiations, %d with changed resources (*), %d lose a wave per SIMD, %d gain scratch'
          % (total, changed, lost, scratch))


if __name__ == '__main__':
    main()
