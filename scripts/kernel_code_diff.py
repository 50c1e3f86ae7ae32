#!/usr/bin/env python3
"""Is the gfx950 device code of two builds of one object (.o / .so) the same?  Compares, kernel by
kernel, the compiler's resource rows (scripts/kernel_resources.py: registers, scratch, LDS, code
size) and the disassembly of every device symbol, the `__hip_cuid_*` hash apart.

    python scripts/kernel_code_diff.py parent/gram_loss.o soft_contrastive_learning_amd/csrc/gram_loss.o

--map FILE: kernels that were renamed between the builds.  Lines `old name<TAB>new name`, the names
as kernel_resources.py prints them (demangled, no parameter list); the first object's symbols take
the second's names before they are matched.  A symbol that differs in at most 8 lines has them shown.

--pcrel: a kernel reaches a module-level constant (scl_cdna4.h: zero_block) by an offset from its own
program counter, so MOVING a kernel inside the module, or into another one, changes that literal and
no instruction.  With this option the literal of the `s_add_u32 sA, sA, <literal>` right behind an
`s_getpc_b64 s[A:A+1]` and the carry operand of the `s_addc_u32 sA+1, sA+1, ...` behind that compare
as equal; registers and every other line, the resource rows and the set of symbols count as before.
The masked lines are counted per symbol, and the symbol order is reported but is no difference.

--subset: the second object may hold only some of the first one's symbols (a source file split in
two): the symbols both have are compared, the others listed.  A symbol that only the second has is
a difference as before.

Exit status 0: identical.  1: the differing kernels are listed with their resource rows.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as K  # noqa: E402


def symbols(txt):
    """(disassembly lines by symbol, symbol order) of llvm-objdump's text"""
    txt = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid', txt)
    txt = re.sub(r'[ \t]*// [0-9A-F]{12}:.*', '', txt)           # the address column of branch targets' lines
    syms, order, cur = {}, [], None
    for line in txt.splitlines():
        m = re.match(r'<(\S+)>:$', line)
        if m:
            cur = m.group(1)
            order.append(cur)
            syms[cur] = []
        elif cur:
            syms[cur].append(line)
    for body in syms.values():      # the zero padding behind whichever symbol comes LAST in .text ("\t\t...")
        while body and body[-1].strip() in ('', '...'):
            body.pop()
    return syms, order


def device_code(path):
    """(resource rows by kernel, disassembly by symbol, symbol order) of the object's code object"""
    with tempfile.TemporaryDirectory() as tmp:
        cos = K.code_objects(path, tmp)
        assert len(cos) == 1, (path, cos)
        rows = {r[0]: r[1:] for r in K.kernels(cos[0])}
        txt = subprocess.run([os.path.join(K.LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn',
                              '--no-leading-addr', cos[0]], capture_output=True, text=True, check=True).stdout
    return (rows,) + symbols(txt)


def mask_pcrel(body):
    """(`body` with the PC-relative offsets masked, the number of lines that changed)"""
    out, n = list(body), 0
    for i, line in enumerate(body):
        m = re.match(r'\s*s_getpc_b64 s\[(\d+):(\d+)\]$', line)
        if not m or int(m.group(2)) != int(m.group(1)) + 1:
            continue
        for j, op, reg in ((i + 1, 's_add_u32', m.group(1)), (i + 2, 's_addc_u32', m.group(2))):
            if j >= len(body):
                break
            lit = re.match(r'(\s*%s s%s, s%s, )(0x[0-9a-f]+|-?\d+)$' % (op, reg, reg), body[j])
            if not lit:
                break           # (no carry line without the add in front of it)
            out[j] = lit.group(1) + '<pcrel>'
            n += 1
    return out, n


def compare(a, b, pcrel=False, subset=False):
    """a, b: (rows, disassembly by symbol, order).  -> (the symbols that differ or that one side lacks,
    the symbols left uncompared because only `a` has them, masked lines of `a` by symbol)"""
    only_a = [s for s in a[2] if s not in b[1]] if subset else []
    bad = sorted(s for s in set(a[1]) ^ set(b[1]) if s not in only_a)
    masked = {}
    for s in a[2]:
        if s not in b[1]:
            continue
        ta, tb = a[1][s], b[1][s]
        if pcrel:
            (ta, masked[s]), (tb, _) = mask_pcrel(ta), mask_pcrel(tb)
        if ta != tb or a[0].get(s) != b[0].get(s):
            bad.append(s)
    return bad, only_a, masked


def renamed(a, b, path):
    """`a` with the symbols that the map file names under their new names, which are symbols of `b`"""
    pairs = dict(line.rstrip('\n').split('\t') for line in open(path) if line.strip())
    short = lambda syms: [K.short_name(n) for n in K.demangle(syms)]
    new_sym = dict(zip(short(b[2]), b[2]))
    old = short(a[2])
    lost = [n for n in pairs if n not in old or pairs[n] not in new_sym]
    assert not lost, 'map lines that name no symbol: %s' % lost
    to = {s: new_sym[pairs[n]] for s, n in zip(a[2], old) if n in pairs}
    return ({to.get(s, s): v for s, v in a[0].items()}, {to.get(s, s): v for s, v in a[1].items()},
            [to.get(s, s) for s in a[2]])


def main():
    argv = sys.argv[1:]
    mapfile = argv.pop(argv.index('--map') + 1) if '--map' in argv else None
    pcrel, subset = '--pcrel' in argv, '--subset' in argv
    argv = [x for x in argv if x not in ('--map', '--pcrel', '--subset')]
    a, b = device_code(argv[0]), device_code(argv[1])
    if mapfile:
        a = renamed(a, b, mapfile)
    bad, only_a, masked = compare(a, b, pcrel, subset)
    same_order = [s for s in a[2] if s not in only_a] == b[2]
    print('%d device symbols / %d kernels in %s, %d / %d in %s; symbol order %s'
          % (len(a[2]), len(a[0]), argv[0], len(b[2]), len(b[0]), argv[1], 'equal' if same_order else 'DIFFERS'))
    for s in bad:
        print('DIFFERS  %s\n   resources (vgpr, agpr, sgpr, scratch, lds, code bytes): %s -> %s'
              % (K.demangle([s])[0], a[0].get(s), b[0].get(s)))
        lines = [d for d in difflib.unified_diff(a[1].get(s, []), b[1].get(s, []), lineterm='', n=0)
                 if d[0] in '+-' and d[:3] not in ('+++', '---')]
        if s in a[1] and s in b[1] and len(lines) <= 8:
            print('\n'.join('   ' + d for d in lines))
    if only_a:
        print('%d symbols of %s compared, %d only it has:' % (len(a[2]) - len(only_a), argv[0], len(only_a)))
        print('\n'.join('   only in the first  %s' % n for n in K.demangle(only_a)))
    if pcrel:
        print('PC-relative offsets masked (lines per symbol), %d in all:' % sum(masked.values()))
        print('\n'.join('   %4d  %s' % (masked[s], n) for s, n in zip(masked, K.demangle(list(masked)))))
    what = 'resource rows and disassembly of every symbol' + (' both have' if only_a else '') + \
        (', PC-relative offsets apart' if pcrel else '')
    if not bad and same_order:
        print('identical: ' + what)
    elif not bad:
        print('identical apart from the symbol order: ' + what)
    return 1 if bad or not (same_order or pcrel) else 0


if __name__ == '__main__':
    sys.exit(main())
