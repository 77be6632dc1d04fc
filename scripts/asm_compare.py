"""Compare the gfx950 code of kernels in two versions of a translation unit (compiled with the library's flags, device side only).

    python scripts/asm_compare.py OLD.hip NEW.hip 'OLD_NAME_REGEX=NEW_NAME_TEMPLATE' [...]

OLD.hip and NEW.hip are paths (each is compiled with its own directory's headers).  Kernels are matched by demangled name: every old
kernel whose name matches OLD_NAME_REGEX is compared with the new kernel named by NEW_NAME_TEMPLATE (re.sub syntax), e.g.

    'decode_attn_owned_kernel<(\\d+)>=decode_attn_kernel<\\1, true>'

Per pair: the registers, LDS, scratch and occupancy the compiler reports for both sides, and the verdict on the instruction streams
after dropping comments and directives and renumbering the basic-block labels in order of appearance: "identical", "identical but
kernarg offset" (the differing lines are scalar loads that differ in their offset alone), "same instructions in the same order,
register numbers differ" (line for line the same opcode and operands but for which register holds a value, the renaming being
one to one within each line), or the number of differing lines."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (('VGPRs', 'NumVgprs'), ('SGPRs', 'TotalNumSgprs'), ('LDS', 'LDSByteSize'), ('scratch', 'ScratchSize'), ('occupancy', 'Occupancy'))


def kernels(src):
    """{demangled name without the parameter list: (instruction lines, resources)} of one source file"""
    from symbolic_music_generation_amd import build as B
    out = os.path.join(tempfile.mkdtemp(prefix='asm_compare_'), 'x.s')
    cmd = [B.HIPCC] + B.FLAGS + B.EXTRA_FLAGS.get(os.path.basename(src), []) + ['-S', '--cuda-device-only', os.path.abspath(src), '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    s = open(out).read()
    names = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', s, re.M)
    plain = subprocess.run(['c++filt'] + names, capture_output=True, text=True, check=True).stdout.split('\n')
    found = {}
    for name, dem in zip(names, plain):
        rest = s.split('\n' + name + ':', 1)[1]             # (the "; Kernel info" comments follow .end_amdhsa_kernel)
        body = rest.split('.end_amdhsa_kernel', 1)[0]
        code, labels = [], {}
        for line in body.split('.section', 1)[0].splitlines():
            t = line.split(';', 1)[0].strip()
            if not t or (t[0] == '.' and not t.startswith('.LBB')):
                continue
            code.append(t)
        for m in re.finditer(r'\.LBB\d+_\d+', '\n'.join(code)):
            labels.setdefault(m.group(0), '.L%d' % len(labels))
        code = [re.sub(r'\.LBB\d+_\d+', lambda m: labels[m.group(0)], t) for t in code]
        res = {k: int((re.search(r';\s*' + key + r':\s*(\d+)', rest) or [0, -1])[1]) for k, key in RES}
        dem = re.sub(r'^void ', '', dem).replace('(anonymous namespace)::', '')
        found[dem.split('(', 1)[0]] = (code, res)
    return found


def verdict(a, b):
    if a == b:
        return 'identical'
    diff = [l for l in difflib.ndiff(a, b) if l[:2] in ('- ', '+ ')]
    gone, come = [l[2:] for l in diff if l[0] == '-'], [l[2:] for l in diff if l[0] == '+']
    strip = lambda t: re.sub(r',\s*(0x[0-9a-f]+|\d+)$', '', t)
    if len(gone) == len(come) and all(x.startswith('s_load_') and strip(x) == strip(y) for x, y in zip(gone, come)):
        return 'identical but kernarg offset (%d scalar load%s)' % (len(gone), 's' if len(gone) > 1 else '')
    reg = r'\b([vsa])(\d+|\[\d+:\d+\])'
    regs = lambda t: re.sub(reg, r'\1#', strip(t) if t.startswith('s_load_') else t)

    def renamed(x, y):      # the same line but for register numbers, and within the line one old register is one new register
        if regs(x) != regs(y):
            return False
        pairs = set(zip(re.findall(reg, x), re.findall(reg, y)))
        return len({o for o, _ in pairs}) == len(pairs) == len({n for _, n in pairs})

    if len(a) == len(b) and all(renamed(x, y) for x, y in zip(a, b)):
        return 'same instructions in the same order, register numbers differ in %d lines' % sum(x != y for x, y in zip(a, b))
    return '%d differing lines' % len(diff)


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    print('%-52s %-8s %s   lines' % ('kernel', 'side', '  '.join('%9s' % k for k, _ in RES)))
    for pair in sys.argv[3:]:
        pat, tmpl = pair.split('=', 1)
        for name in sorted(n for n in old if re.fullmatch(pat, n)):
            other = re.sub(pat, tmpl, name)
            if other not in new:
                sys.exit('no kernel %s in %s' % (other, sys.argv[2]))
            for side, n, k in (('parent', name, old[name]), ('this', other, new[other])):
                print('%-52s %-8s %s   %d' % (n, side, '  '.join('%9d' % k[1][key] for key, _ in RES), len(k[0])))
            print('    -> ' + verdict(old[name][0], new[other][0]))
            if os.environ.get('ASM_DIFF'):              # ASM_DIFF=n: the first n lines of the unified diff as well
                print('\n'.join(list(difflib.unified_diff(old[name][0], new[other][0], lineterm='', n=2))[:int(os.environ['ASM_DIFF'])]))


if __name__ == '__main__':
    main()
