"""Diagnostic: where the step loop of one split-form instance issues its row loads, as compiled.

    python scripts/lt_issue_points.py "2, 2, false, 4, 1, 8, 2, 0" [--lib <libfedsim.so>] [--rate 1/1] [--tail 0/2]

(template arguments RT, G, PROX, EARLY, TEAMS, WAVES, TPWK, MBK of local_train_split_kernel).  The
gfx950 code objects are taken out of the built library, the instance is disassembled with
llvm-objdump, and of its instructions only four mnemonics are read: v_mfma*, global_load_dwordx4,
s_barrier and s_waitcnt with a vmcnt.  Printed:
  pattern   the step loop in order: [n] = a run of n MFMAs, L = a row load, B = s_barrier,
            vmcnt(n) = a wait.  The step is found as the three barriers S1, S2, S3 with no MFMA
            between them; it runs from the first MFMA after the barrier ahead of S1 to the waits
            behind the last MFMA.
  loads     for every row load behind S3: the backward MFMA after which it issues, and the MFMA
            after which the source asks for it (`--rate` = SP_BWD_NUM / SP_BWD_DEN loads per
            backward iteration of the 16x16x4 instances at G = 2, `--tail` = SP_BWD_TAIL / SP_BWD_TAILPER, its
            last loads at the backward's end; the mb instances issue TPWK per row block)
  spill     the instance's VGPR spill count and scratch bytes from the code object's metadata
A listing file made with `llvm-objdump -d` (or hipcc -S) can be given instead of a library: --asm.
"""
import argparse
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'non-iid-distributed-learning-with-optimal-mixture-weights_amd')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def tool(name):
    for p in (shutil.which(name), '/opt/rocm/llvm/bin/' + name, '/opt/rocm/lib/llvm/bin/' + name):
        if p and os.path.exists(p):
            return p
    return None


def parse_args_str(s):
    v = [x.strip() for x in s.split(',')]
    if len(v) != 8:
        raise SystemExit('instance: 8 template arguments RT, G, PROX, EARLY, TEAMS, WAVES, TPWK, MBK')
    prox = v[2] in ('true', '1')
    n = [int(x) for x in v[:2] + v[3:]]
    return dict(RT=n[0], G=n[1], PROX=prox, EARLY=n[2], TEAMS=n[3], WAVES=n[4], TPWK=n[5], MBK=n[6])


def mangled(a):
    return ('_ZN2fs24local_train_split_kernelILi%dELi%dELb%dELi%dELi%dELi%dELi%dELi%dEEEvNS_8LTParamsENS_7SplitWSE'
            % (a['RT'], a['G'], int(a['PROX']), a['EARLY'], a['TEAMS'], a['WAVES'], a['TPWK'], a['MBK']))


def code_objects(lib, arch='gfx950'):
    """the device code objects of `arch` bundled in a host library (uncompressed clang offload bundles)"""
    blob = open(lib, 'rb').read()
    out, pos = [], 0
    while True:
        pos = blob.find(MAGIC, pos)
        if pos < 0:
            break
        p = pos + len(MAGIC)
        (n,) = struct.unpack_from('<Q', blob, p)
        p += 8
        if n > 64:       # the magic inside a string, not a bundle header
            pos += 1
            continue
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', blob, p)
            p += 24
            triple = blob[p:p + tl].decode('ascii', 'replace')
            p += tl
            if triple.startswith('hip') and triple.endswith(arch) and size:
                out.append(blob[pos + off:pos + off + size])
        pos += 1
    return out


def disassemble(lib, sym):
    """(listing of `sym`, metadata text of its code object) from the library"""
    objdump, readelf = tool('llvm-objdump'), tool('llvm-readelf')
    if not objdump:
        raise SystemExit('llvm-objdump not found')
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(code_objects(lib)):
            if sym.encode() not in co:
                continue
            path = os.path.join(td, 'co%d.o' % k)
            with open(path, 'wb') as f:
                f.write(co)
            txt = subprocess.run([objdump, '-d', '--no-show-raw-insn', '--disassemble-symbols=' + sym, path],
                                 check=True, capture_output=True, text=True).stdout
            meta = ''
            if readelf:
                meta = subprocess.run([readelf, '--notes', path], check=True, capture_output=True, text=True).stdout
            return txt, meta
    raise SystemExit('no gfx950 code object of %s holds %s' % (lib, sym))


def events(listing, sym=None):
    """the four mnemonics of a listing, in order: ('M',), ('L',), ('B',), ('W', n).  In a whole-file
    assembly listing only the lines of `sym` (label to .Lfunc_end) are read."""
    ev, on = [], sym is None or (sym + ':') not in listing
    for line in listing.splitlines():
        s = line.strip()
        if not on:
            on = s.startswith(sym + ':')
            continue
        if sym and s.startswith('.Lfunc_end'):
            break
        s = re.sub(r'^[0-9a-fA-F]+:\s*', '', s)       # objdump's address column, if any
        m = s.split(None, 1)
        if not m:
            continue
        op = m[0]
        if op.startswith('v_mfma'):
            ev.append(('M',))
        elif op == 'global_load_dwordx4':
            ev.append(('L',))
        elif op == 's_barrier':
            ev.append(('B',))
        elif op == 's_waitcnt':
            w = re.search(r'vmcnt\((\d+)\)', s)
            if w:
                ev.append(('W', int(w.group(1))))
    return ev


def step_loop(ev):
    """(first, s3, last): indices of the step's first event, its S3 barrier and its last event"""
    bars = [k for k, e in enumerate(ev) if e[0] == 'B']
    has_m = lambda a, b: any(e[0] == 'M' for e in ev[a:b])
    for x in range(len(bars) - 2):
        s1, s2, s3 = bars[x], bars[x + 1], bars[x + 2]
        prev = bars[x - 1] if x > 0 else -1
        nxt = bars[x + 3] if x + 3 < len(bars) else len(ev)
        if has_m(prev + 1, s1) and not has_m(s1, s3) and has_m(s3, nxt):
            first = next(k for k in range(prev + 1, s1) if ev[k][0] == 'M')
            lastm = max(k for k in range(s3, nxt) if ev[k][0] == 'M')
            last = lastm
            while last + 1 < nxt and ev[last + 1][0] == 'W':      # the step-end waits
                last += 1
            return first, s3, last
    raise SystemExit('step loop not found (three barriers without an MFMA between them)')


def pattern(ev):
    out, n = [], 0
    for e in ev:
        if e[0] == 'M':
            n += 1
            continue
        if n:
            out.append('[%d]' % n)
            n = 0
        out.append({'L': 'L', 'B': 'B'}.get(e[0]) or 'vmcnt(%d)' % e[1])
    if n:
        out.append('[%d]' % n)
    return ' '.join(out)


def source_points(a, num, den, tail=0, tailper=2):
    """backward MFMA after which the source issues each in-backward row load, and the backward's MFMAs"""
    nld = a['TPWK'] * 4 * a['RT']
    ne = min(a['EARLY'], nld)
    pts = []
    if a['MBK'] == 0:
        nit, per = a['TPWK'] * 4 * a['RT'], 4
        fenced = (a['RT'] == 2 and a['G'] == 2 and not a['PROX'] and a['TEAMS'] == 1 and a['TPWK'] > 1
                  and 0 < ne < nld)
        for f in range(ne, nld):
            if not fenced:
                it = f - ne
            elif f < nld - tail:          # the stream's head: num / den loads per iteration
                it = min(((f - ne + 1) * den + num - 1) // num - 1, nit - 1)
            else:                         # its last `tail` loads: tailper per iteration at the backward's end
                it = nit - 1 - (nld - 1 - f) // tailper
            pts.append((it + 1) * per)
    else:
        nit, per = 4 * a['RT'], 4 * a['TPWK'] * a['MBK']
        for kk in range(nit):
            for i in range(a['TPWK']):
                if kk * a['TPWK'] + i + ne < nld:
                    pts.append((kk + 1) * per)
    return pts, nit * per


def spill(meta, sym):
    """(vgpr spill count, scratch bytes) of `sym` from `llvm-readelf --notes` output, or None"""
    blocks = re.split(r'\n\s*- \.agpr_count:', meta)
    for b in blocks:
        if re.search(r'\.name:\s*' + re.escape(sym) + r'\s*\n', b):
            v = re.search(r'\.vgpr_spill_count:\s*(\d+)', b)
            p = re.search(r'\.private_segment_fixed_size:\s*(\d+)', b)
            return (int(v.group(1)) if v else None, int(p.group(1)) if p else None)
    return None


def report(a, listing, meta, num, den, sym, tail=0, tailper=2):
    ev = events(listing, sym)
    first, s3, last = step_loop(ev)
    lines = ['instance  local_train_split_kernel<%d,%d,%s,%d,%d,%d,%d,%d>'
             % (a['RT'], a['G'], 'true' if a['PROX'] else 'false', a['EARLY'], a['TEAMS'], a['WAVES'], a['TPWK'], a['MBK'])]
    lines.append('pattern   ' + pattern(ev[first:last + 1]))
    lines.append('after S3  ' + pattern(ev[s3 + 1:last + 1]))
    pts, nb = source_points(a, num, den, tail, tailper)
    at, m = [], 0
    for e in ev[s3 + 1:last + 1]:
        if e[0] == 'M':
            m += 1
        elif e[0] == 'L':
            at.append(m)
    lines.append('backward  %d MFMAs; %d row loads behind S3 (the source issues %d)' % (nb, len(at), len(pts)))
    worst = 0
    for k, m in enumerate(at):
        src = pts[k] if k < len(pts) else None
        late = m - src if src is not None else None
        if late is not None:
            worst = max(worst, abs(late))
        lines.append('load %2d   issued after backward MFMA %3d, source after %s%s'
                     % (k, m, '%3d' % src if src is not None else '  -', '  (%+d)' % late if late else ''))
    lines.append('worst     %d MFMAs from the source point' % worst)
    sp = spill(meta, sym) if meta else None
    if sp:
        lines.append('spill     VGPR spill count %s, scratch %s bytes per lane' % sp)
    return lines, dict(issued=at, source=pts, worst=worst, spill=sp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('instance', help='"RT, G, PROX, EARLY, TEAMS, WAVES, TPWK, MBK"')
    ap.add_argument('--lib', default=os.path.join(PKG, 'libfedsim.so'))
    ap.add_argument('--asm', help='a listing of the instance (llvm-objdump -d / hipcc -S) instead of a library')
    ap.add_argument('--rate', default='1/1', help='SP_BWD_NUM/SP_BWD_DEN the library was built with')
    ap.add_argument('--tail', default='0/2', help='SP_BWD_TAIL/SP_BWD_TAILPER the library was built with')
    o = ap.parse_args()
    a = parse_args_str(o.instance)
    num, den = [int(x) for x in o.rate.split('/')]
    tail, tailper = [int(x) for x in o.tail.split('/')]
    sym = mangled(a)
    if o.asm:
        listing, meta = open(o.asm).read(), ''
    else:
        listing, meta = disassemble(o.lib, sym)
    lines, _ = report(a, listing, meta, num, den, sym, tail, tailper)
    print('\n'.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
