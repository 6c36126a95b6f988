#!/usr/bin/env python3
"""Resource table of every kernel instantiation of some .hip files, parent -> branch:
  scripts/kernel_resources.py <parent tree> <branch tree> "<title>" [--files a.hip b.hip ...]
      [--kernels REGEX] [--rename REGEX REPLACEMENT] [--new REGEX REPLACEMENT]
      [--flags extra hipcc flags of the branch]
      > profiles/<name>.txt
Compiles the files (default: hmc_gauss.hip, hmc_gauss_rng.hip, hmc_gauss_rng_wide.hip; for the
pair-distance model: --files pairdist.hip --kernels .) of both trees for the device alone with
-S -Rpass-analysis=kernel-resource-usage and prints, per kernel whose demangled name matches
--kernels (default: hmc_gauss_persist_kernel), VGPRs, SGPRs, scratch and occupancy of both, and
whether the kernel's instruction stream equals the parent's: a digest of the function's text
in the assembly between its label and its end, with comments, directives and blank lines
stripped and local labels numbered in order of appearance.  --rename maps a parent's kernel
name to the branch's where a pull request renames one; --new maps the name of a kernel that only
the branch instantiates to the parent's kernel it is set against (a new template parameter's
variant against the kernel it would replace: "new" in the code column).  The last lines count
what changed.
No GPU needed."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

GAUSS_FILES = ['hmc_gauss.hip', 'hmc_gauss_rng.hip', 'hmc_gauss_rng_wide.hip']
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '--cuda-device-only',
         '-Rpass-analysis=kernel-resource-usage', '-S']


def demangle(names):
    """{mangled: 'binf::kernel<16, true>'}: the parameter list and the return type dropped."""
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt')
    if not filt or not names:
        return {n: n for n in names}
    out = subprocess.run([filt], input='\n'.join(names), text=True, capture_output=True, check=True).stdout
    res = {}
    for n, d in zip(names, out.splitlines()):
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):
            depth += (ch == '<') - (ch == '>')
            if ch == '(' and depth == 0 and not d.startswith('(anonymous namespace)', i):
                cut = i
                break
        res[n] = re.sub(r'^void ', '', d[:cut])
    return res


def stream_digests(asm):
    """{mangled: digest of the function's instructions}."""
    res, cur, body, labels = {}, None, [], {}
    for line in asm.splitlines():
        if cur is None:
            m = re.match(r'^(_Z\w+):', line)
            if m:
                cur, body, labels = m.group(1), [], {}
            continue
        if line.startswith('.Lfunc_end'):
            text = '\n'.join(body)
            text = re.sub(r'\.LBB\d+_\d+', lambda m: '.L%d' % labels.get(m.group(0), -1), text)
            res[cur] = hashlib.sha256(text.encode()).hexdigest()[:12]
            cur = None
            continue
        m = re.match(r'^(\.LBB\d+_\d+):', line)
        if m:
            labels[m.group(1)] = len(labels)
            body.append('.L%d:' % labels[m.group(1)])
            continue
        line = line.split(';')[0].strip()
        if not line or line.startswith('.') or line.endswith(':'):
            continue
        body.append(re.sub(r'\s+', ' ', line))
    return res


def resources(tree, name, extra, pattern):
    with tempfile.TemporaryDirectory() as tmp:
        asm_path = os.path.join(tmp, 'out.s')
        err = subprocess.run([HIPCC] + FLAGS + extra + [os.path.join(tree, 'binf_amd', 'csrc', name), '-o', asm_path],
                             text=True, capture_output=True, check=True).stderr
        asm = open(asm_path).read()
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
    digests = stream_digests(asm)
    names = demangle(list(res))
    table = {}
    for k, v in res.items():
        if re.search(pattern, names[k]):
            v['stream'] = digests.get(k, '?')
            table[names[k]] = v
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parent')
    ap.add_argument('branch')
    ap.add_argument('title')
    ap.add_argument('--files', nargs='+', default=GAUSS_FILES)
    ap.add_argument('--kernels', default='hmc_gauss_persist_kernel')
    ap.add_argument('--rename', nargs=2, action='append', default=[], metavar=('REGEX', 'REPLACEMENT'))
    ap.add_argument('--new', nargs=2, action='append', default=[], metavar=('REGEX', 'REPLACEMENT'))
    ap.add_argument('--flags', nargs=argparse.REMAINDER, default=[])
    o = ap.parse_args()
    jobs = [(t, f) for f in o.files for t in (o.parent, o.branch)]
    with ThreadPoolExecutor(max_workers=6) as ex:
        got = list(ex.map(lambda j: resources(j[0], j[1], o.flags if j[0] == o.branch else [], o.kernels), jobs))
    print('kernels matching /%s/: -Rpass-analysis=kernel-resource-usage and instruction streams, parent -> %s'
          % (o.kernels, o.title))
    print('(every instantiation; v = VGPRs, s = SGPRs, scr = scratch bytes per lane, occ = waves per SIMD,')
    print(' code = whether the instruction stream equals the parent\'s; * = changed resources)')
    total = changed = lost = scratch = differ = added = 0
    for i, f in enumerate(o.files):
        a, b = got[2 * i], got[2 * i + 1]
        for pat, rep in o.rename:
            a = {re.sub(pat, rep, k): v for k, v in a.items()}
        print('\n== %s' % f)
        against = {}
        for k in b:
            if k not in a:
                for pat, rep in o.new:
                    if re.search(pat, k) and re.sub(pat, rep, k) in a:
                        against[k] = re.sub(pat, rep, k)
        assert sorted(a) == sorted(k for k in b if k not in against), \
            'the two trees instantiate different kernels in %s: %s' % (f, sorted((set(a) ^ set(b)) - set(against)))
        for k in b:
            x, y = dict(a[against.get(k, k)]), dict(b[k])
            same = x.pop('stream') == y.pop('stream')
            total += 1
            changed += x != y
            differ += not same and k not in against
            added += k in against
            lost += y['occ'] < x['occ']
            scratch += y['scr'] > x['scr']
            print('%-70s v %3d->%3d s %3d->%3d scr %d->%d occ %d->%d code %s%s' % (
                k, x['v'], y['v'], x['s'], y['s'], x['scr'], y['scr'], x['occ'], y['occ'],
                'new' if k in against else 'same' if same else 'DIFFERS', '   *' if x != y else ''))
    print('\n%d instantiations, %d with changed resources (*), %d lose a wave per SIMD, %d gain scratch, '
          '%d with a different instruction stream, %d new (set against the kernel they stand in for)'
          % (total, changed, lost, scratch, differ, added))


if __name__ == '__main__':
    main()
