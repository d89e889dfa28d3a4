"""DEVELOPER-ONLY: per-kernel instruction mix from `hipcc -S --cuda-device-only` output.  Usage: isa_mix.py file.s [name-substring ...]

kernel_mix(text) is the parser (tests/test_lds_single_reads_compile.py counts LDS reads with it)."""
import collections
import re
import sys


def kernel_mix(s, want=()):
    """assembly text -> {mangled kernel name: Counter of mnemonics}, for the kernels whose name holds one of `want` (all if empty)"""
    out = {}
    starts = [(m.start(), m.group(1)) for m in re.finditer(r'^(_Z\w+):', s, re.M)]
    for i, (pos, name) in enumerate(starts):
        if want and not any(w in name for w in want):
            continue
        end = starts[i + 1][0] if i + 1 < len(starts) else len(s)
        body = s[pos:end].split('.end_amdhsa_kernel')[0]
        ins = [l.split()[0] for l in body.split('\n') if l.strip() and l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;")]
        out[name] = collections.Counter(ins)
    return out


def main(argv):
    for name, c in kernel_mix(open(argv[1]).read(), argv[2:]).items():
        grp = lambda p: sum(v for k, v in c.items() if k.startswith(p))
        print("%s\n  total %d  valu %d (pk %d)  ds %d  global/buffer %d  scratch %d  salu %d  waitcnt %d" % (
            name[:70], sum(c.values()), grp('v_'), grp('v_pk'), grp('ds_'), grp('global_') + grp('buffer_'), grp('scratch_'), grp('s_') - c['s_waitcnt'] - c['s_nop'], c['s_waitcnt']))
        print("  ", ", ".join("%s %d" % kv for kv in c.most_common(24)))


if __name__ == "__main__":
    main(sys.argv)
