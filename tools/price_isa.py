#!/usr/bin/env python3
"""Price a kernel's hottest loop with the measured gfx950 VALU issue costs (tools/issue_probe.py,
profiles/r01_valu_issue_costs.txt: cycles per wave-instruction per SIMD and the clock the SIMD held, 8 waves per SIMD,
varying data).
usage: price_isa.py file.s kernel_substring [--loops] [--span=VALU] [--clock=MHZ]
--loops: one line per loop of the kernel (innermost backward-branch spans, largest first) instead of the hottest alone,
         with the operand forms of its FMAs.
--span=N: price the loop whose span holds N VALU instructions (as --loops lists them) instead of the largest.
--clock=MHZ: the clock the kernel held (bench.py: roofline.executed.clock_mhz_held) for the ns line; default 2200.

An instruction with an SGPR source, or one of the second pipe's (v_max, v_cmp, v_cndmask, v_cvt, ...), costs 4.1 cycles in
a stream of its like and ~2.1 when it stands alone among full-rate instructions (fma+mul(sgpr), 2fma+max, cmp+cnd+2fma in
the table).  Each is therefore priced by its place: interleaved if the VALU instruction before it is a full-rate one,
alone if it follows another of its class; the two bounds (all interleaved, all alone) are printed as well.
The ns line weighs each form by the clock its probe held, scaled to --clock: a three-register v_fma_f32 stream held
1894 MHz where v_fmaak held 2218 and SGPR-source forms 2370.  So far the model's DIFFERENCES between two builds of a
loop, not its absolute value, have matched what was measured (literal forms 0.8 % priced, 0.7 % measured;
the spin constants in SGPRs 1.0 % priced by place, 2.1 % as all interleaved, 1.2 % measured)."""
import re, sys, collections
s = open(sys.argv[1]).read()
key = sys.argv[2]
m = re.search(r'^(_Z[^\n]*' + re.escape(key) + r'[^\n]*):[^\n]*\n(.*?)\.Lfunc_end', s, re.S | re.M)
body = m.group(2).split('\n')
# find loops: label ... s_cbranch back to label; choose the largest backward-branch span
labels = {}
for i, l in enumerate(body):
    mm = re.match(r'^(\.LBB\S+):', l)
    if mm: labels[mm.group(1)] = i
best = None
for i, l in enumerate(body):
    mm = re.search(r's_cbranch_\w+\s+(\.LBB\S+)', l)
    if mm and mm.group(1) in labels and labels[mm.group(1)] < i:
        span = (labels[mm.group(1)], i)
        if best is None or span[1] - span[0] > best[1] - best[0]: best = span
if '--loops' in sys.argv[3:]:
    # every backward branch, conditional or not (a rotated loop closes with s_branch), is a loop; nested ones (the tile
    # loop around the step loops) are listed too
    spans = sorted({(labels[mm.group(1)], i) for i, l in enumerate(body)
                    for mm in [re.search(r's_c?branch\w*\s+(\.LBB\S+)', l)] if mm and mm.group(1) in labels and labels[mm.group(1)] < i},
                   key=lambda sp: sp[0] - sp[1])
    for a, b in spans:
        ops = [l.strip().split()[0] for l in body[a:b + 1] if l.strip() and not l.strip().startswith(('.', ';')) and not l.strip().endswith(':')]
        n_valu = sum(o.startswith('v_') for o in ops)
        ls = [l.strip() for l in body[a:b + 1] if l.strip().startswith('v_')]
        sg = lambda l: bool(re.search(r'(^|[ ,-])s\d+', l.split(None, 1)[1])) if ' ' in l else False
        fma, fmac = [l for l in ls if l.startswith('v_fma_f32')], [l for l in ls if l.startswith('v_fmac_f32')]
        print(f"loop lines {a}-{b}: {len(ops)} instructions, VALU {n_valu}, v_rndne {sum(o.startswith('v_rndne') for o in ops)}, "
              f"v_cvt {sum(o.startswith('v_cvt') for o in ops)}, v_pk {sum(o.startswith('v_pk_') for o in ops)}; "
              f"v_fma_f32 three VGPRs {sum(l.split(None, 1)[1].count('v') == 4 for l in fma)} / SGPR source {sum(map(sg, fma))}, "
              f"v_fmac_f32 plain {sum(not sg(l) for l in fmac)} / SGPR source {sum(map(sg, fmac))}")
    sys.exit(0)
want = [int(x.split('=')[1]) for x in sys.argv[3:] if x.startswith('--span=')]
if want:
    for i, l in enumerate(body):
        mm = re.search(r's_c?branch\w*\s+(\.LBB\S+)', l)
        if mm and mm.group(1) in labels and labels[mm.group(1)] < i:
            if sum(x.strip().startswith('v_') for x in body[labels[mm.group(1)]:i + 1]) == want[0]: best = (labels[mm.group(1)], i)
lo, hi = best
ins = [l.strip().split()[0] for l in body[lo:hi + 1] if l.strip() and not l.strip().startswith(('.', ';')) and not l.strip().endswith(':')]
full = lambda l: l
lines = [l.strip() for l in body[lo:hi + 1] if l.strip() and not l.strip().startswith(('.', ';')) and not l.strip().endswith(':')]
HALF = ('v_max', 'v_min', 'v_cmp', 'v_rndne', 'v_cvt', 'v_cndmask', 'v_floor', 'v_trunc', 'v_med3', 'v_fract', 'v_ldexp', 'v_frexp',
        'v_lshl', 'v_bfi')
TRANS = ('v_rcp', 'v_sqrt', 'v_rsq', 'v_sin', 'v_cos', 'v_exp', 'v_log')
# form -> (cycles, MHz) at 8 waves per SIMD, varying data (profiles/r01_valu_issue_costs.txt)
FULL = {'v_fma_f32': (2.20, 1894), 'v_fmac': (2.30, 2178), 'v_mul': (2.34, 2230), 'v_add': (2.33, 2321), 'v_sub': (2.33, 2321),
        'v_fmaak': (2.20, 2218), 'v_fmamk': (2.24, 2241), 'v_mov': (2.35, 2356), 'v_and': (2.33, 2245), 'v_xor': (2.38, 2188)}
FULL_OTHER = (2.3, 2250)
ALONE = {'sgpr': (4.1, 2370), 'half': (4.1, 2390)}       # v_fma_f32(sgpr) 4.12 / 2368, v_fmac 4.09 / 2377, v_mul 4.10 / 2378; v_max 4.12 / 2390
MIXED = {'sgpr': (2.16, 2277), 'half': (2.10, 2280)}     # fma+mul(sgpr) 2.16 / 2277; 2fma+max 2.12 / 2246, cmp+cnd+2fma 2.08 / 2292, 3fma+cvt 2.09 / 2300
held = ([float(x.split('=')[1]) for x in sys.argv[3:] if x.startswith('--clock=')] or [2200.0])[0]
cls = collections.Counter(); cyc = collections.Counter(); ns = collections.Counter()
lo_cyc = hi_cyc = lo_ns = hi_ns = 0.0
prev_full = True
for l in lines:
    op = l.split()[0]
    if not op.startswith('v_'):
        cls['salu/other'] += 1; continue
    args = l.split(None, 1)[1] if ' ' in l else ''
    second = None
    if op.startswith(TRANS): k, (c, mhz) = 'trans', (8.1, 2390)
    elif op.startswith('v_pk_'): k, (c, mhz) = 'packed', (4.4, 1853)
    elif op.startswith(HALF): second = 'half'
    elif op.startswith(('v_fma_f32', 'v_fmac', 'v_mul', 'v_add', 'v_sub', 'v_mad')) and re.search(r'(^|[ ,-])s\d+', args): second = 'sgpr'
    else: k, (c, mhz) = 'full', next((v for p, v in FULL.items() if op.startswith(p)), FULL_OTHER)
    if second:
        k = second + (' interleaved' if prev_full else ' in a run')
        c, mhz = (MIXED if prev_full else ALONE)[second]
        lo_cyc += MIXED[second][0]; lo_ns += MIXED[second][0] / MIXED[second][1]
        hi_cyc += ALONE[second][0]; hi_ns += ALONE[second][0] / ALONE[second][1]
    else:
        lo_cyc += c; hi_cyc += c; lo_ns += c / mhz; hi_ns += c / mhz
    prev_full = k == 'full'
    cls[k] += 1; cyc[k] += c; ns[k] += c / mhz
print(f"loop lines {lo}-{hi}: {len(lines)} instructions, VALU {sum(v for k, v in cls.items() if k != 'salu/other')}")
for k in cls: print(f"  {k:18s} n={cls[k]:4d} cycles={cyc[k]:7.1f}")
cost = sum(cyc.values())
print(f"  priced VALU issue cycles per iteration: {cost:.0f}   (every SGPR-source / second-pipe instruction interleaved: {lo_cyc:.0f}, alone: {hi_cyc:.0f})")
# each form at the clock its probe held, the whole scaled so that the v_fmaak stream's 2218 MHz is --clock
scale = 2218.0 / held
print(f"  priced span at a held clock of {held:.0f} MHz: {sum(ns.values()) * 1e3 * scale:.1f} ns per SIMD with one wave issuing per slot "
      f"(interleaved {lo_ns * 1e3 * scale:.1f}, alone {hi_ns * 1e3 * scale:.1f}); compare two builds' DIFFERENCE, not the value")
c2 = collections.Counter(l.split()[0] for l in lines)
print("  top ops:", ", ".join(f"{k}:{v}" for k, v in c2.most_common(14)))
