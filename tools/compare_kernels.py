#!/usr/bin/env python3
"""Compare two builds of libazg_hip.so kernel by kernel: the set of kernel symbols, the exported symbols (llvm-nm -D's) and -- for the kernels
whose name contains one of the given substrings (default: the asynchronous pipeline's) -- the disassembly and the resource notes (VGPRs,
SGPRs, spills, scratch, LDS).  Per symbol, not per file: the order of instantiation may move functions around inside a code object.
    python tools/compare_kernels.py OLD.so NEW.so [substring ...]
Exit status 0 when everything compared is identical."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_kernel_resources import LLVM, MAGIC, kernel_notes  # noqa: E402


def kernel_text(lib):
    """-> ({mangled symbol: disassembly without addresses, encodings and address comments}, {mangled symbol: the pc-relative literals masked
    in it}) over every gfx950 code object in the library"""
    out, masked = {}, {}
    with tempfile.TemporaryDirectory() as t:
        fat = os.path.join(t, 'fat.bin')
        subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, lib, os.devnull])
        blob = open(fat, 'rb').read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for k, a in enumerate(starts):
            part, co = os.path.join(t, 'b%d.bin' % k), os.path.join(t, 'b%d.co' % k)
            open(part, 'wb').write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--input=' + part,
                                   '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co, '--unbundle'])
            dis = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-leading-addr', '--no-show-raw-insn', co], text=True)
            cur = None
            for ln in dis.splitlines():
                m = re.match(r'^[0-9a-f]* ?<(\S+)>:$', ln)
                if m:
                    cur = m.group(1)
                    out[cur], masked[cur] = [], []
                elif cur is not None:
                    ln = ln.split('//')[0].rstrip()
                    # the literal behind s_getpc_b64 is the DISTANCE from here to a constant table of the code object: it changes whenever
                    # the linker lays the functions out in another order, the instruction does not.  Masked in the text, kept aside:
                    # main() prints every pair that differs, so that nothing changes unseen behind the mask
                    m = re.match(r'^(\s*s_add_u32 \S+ \S+) (0x[0-9a-f]+)$', ln) if out[cur] and 's_getpc_b64' in out[cur][-1] else None
                    if m:
                        ln = m.group(1) + ' <pc-relative>'
                        masked[cur].append(m.group(2))
                    out[cur].append(ln)
    return {k: '\n'.join(v) for k, v in out.items()}, masked


def exported(lib):
    """the defined dynamic symbols (what llvm-nm -D --defined-only lists; read with llvm-readelf, which every ROCm install has)"""
    rows = [ln.split() for ln in subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--dyn-syms', '-W', lib], text=True).splitlines()]
    # (__hip_cuid_<hash>: hipcc's id of a translation unit, a hash over its path and text -- not an interface)
    return [r[7] for r in rows if len(r) == 8 and r[0].rstrip(':').isdigit() and r[6] != 'UND' and not r[7].startswith('__hip_cuid_')]


def main(old, new, *subs):
    subs = subs or ('k_async_select', 'k_async_net', 'k_async_requeue')
    bad = 0
    nm = [exported(lib) for lib in (old, new)]
    print('exported symbols: %d / %d, %s' % (len(nm[0]), len(nm[1]), 'identical' if sorted(nm[0]) == sorted(nm[1]) else 'DIFFERENT'))
    bad += sorted(nm[0]) != sorted(nm[1])
    for s in sorted(set(nm[0]) ^ set(nm[1])):
        print('   only in', 'old' if s in nm[0] else 'new', s)
    notes = [kernel_notes(lib) for lib in (old, new)]
    print('kernel symbols: %d / %d, %s' % (len(notes[0]), len(notes[1]), 'identical' if set(notes[0]) == set(notes[1]) else 'DIFFERENT'))
    bad += set(notes[0]) != set(notes[1])
    for s in sorted(set(notes[0]) ^ set(notes[1])):
        print('   only in', 'old' if s in notes[0] else 'new', s)
    (text0, lit0), (text1, lit1) = kernel_text(old), kernel_text(new)
    text = [text0, text1]
    dem = dict(zip(text[0], subprocess.check_output(['c++filt'] + list(text[0]), text=True).splitlines()))
    n = 0
    for sym in sorted(text[0]):
        d = dem[sym]
        if d not in notes[0] or not any(s in d for s in subs):
            continue
        n += 1
        same_text, same_notes = text[0][sym] == text[1].get(sym), notes[0][d] == notes[1].get(d)
        if lit0[sym] != lit1.get(sym):
            print('   pc-relative literals (distance to a constant table; masked in the text) differ in %s: %s -> %s' % (
                d, ' '.join(lit0[sym]), ' '.join(lit1.get(sym, []))))
        if not (same_text and same_notes):
            bad += 1
            print('   DIFFERENT %s%s: %s' % ('text ' if not same_text else '', 'notes' if not same_notes else '', d))
    print('%d kernels compared (%s): disassembly and resource notes %s' % (n, ', '.join(subs), 'identical' if not bad else 'NOT all identical'))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:]))
