"""Diagnostic: static instruction counts of one split-form instance's hand-off chain, as compiled.

    python scripts/split_chain_isa.py "2, 2, false, 4, 1, 8, 2, 0" [--lib <libfedsim.so>]

(template arguments as scripts/lt_issue_points.py, whose disassembly this reads.)  The step is found
as the three barriers S1, S2, S3 with no MFMA between them; the step loop is the span of the
backward branches around them.  Printed: the instructions, v_readlane_b32 restores and branches from
S1 to S3; integer divisions (v_rcp_iflag_f32) in the step loop; IEEE divisions (v_div_scale_f32)
between S2 and S3; the hand-off's sc1 publish stores and sc1 loads per poll; the instructions from
the loop's head to the first forward MFMA and from S3 to the first backward MFMA; registers, SGPR
spills and scratch from the code object's metadata.
"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lt_issue_points as tool  # noqa: E402


def instructions(listing):
    """[(byte offset in the function, mnemonic, operands, branch target offset or None)]"""
    out, base = [], None
    for line in listing.splitlines():
        m = re.match(r'\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):', line)
        if not m:
            continue
        addr = int(m.group(3), 16)
        if base is None:
            base = addr
        t = re.search(r'<[^>]*\+0x([0-9a-fA-F]+)>\s*$', line) if 'branch' in m.group(1) else None
        out.append((addr - base, m.group(1), m.group(2), int(t.group(1), 16) if t else None))
    return out


def chain(ins):
    """indices (head, s1, s2, s3, end) of the step loop's first instruction, its three barriers and
    its backward branch"""
    bars = [k for k, i in enumerate(ins) if i[1] == 's_barrier']
    mf = lambda a, b: any(i[1].startswith('v_mfma') for i in ins[a:b])
    for x in range(len(bars) - 2):
        s1, s2, s3 = bars[x:x + 3]
        prev = bars[x - 1] if x else 0
        nxt = bars[x + 3] if x + 3 < len(bars) else len(ins)
        if mf(prev, s1) and not mf(s1, s3) and mf(s3, nxt):
            break
    else:
        raise SystemExit('step not found (three barriers without an MFMA between them)')
    off = {i[0]: k for k, i in enumerate(ins)}
    loops = [(off[i[3]], k) for k, i in enumerate(ins) if i[3] is not None and i[3] in off and off[i[3]] <= k]
    around = [(a, b) for a, b in loops if a <= s1 and b >= s3]
    if not around:
        raise SystemExit('no loop around the step')
    # (a rotated loop has several back-edges and latches: the loop is the span of them all)
    return min(a for a, _ in around), s1, s2, s3, max(b for _, b in around)


def polls(ins, a, b):
    """sizes of the groups of sc1 granule loads (one group = one poll) between a and b"""
    at = [k for k in range(a, b) if ins[k][1] == 'global_load_dwordx2' and 'sc1' in ins[k][2]]
    groups = []
    for k in at:
        if groups and k - groups[-1][-1] <= 8:
            groups[-1].append(k)
        else:
            groups.append([k])
    return [len(g) for g in groups]


def metadata(meta, sym):
    for b in re.split(r'\n\s*- \.agpr_count:', meta):
        if re.search(r'\.name:\s*' + re.escape(sym) + r'\s*\n', b):
            f = lambda k: int(re.search(r'\.%s:\s*(\d+)' % k, b).group(1))
            return dict(vgprs=f('vgpr_count'), sgpr_spill=f('sgpr_spill_count'), vgpr_spill=f('vgpr_spill_count'),
                        scratch=f('private_segment_fixed_size'))
    return None


def counts(listing, meta, sym):
    ins = instructions(listing)
    head, s1, s2, s3, end = chain(ins)
    n = lambda a, b, f: sum(1 for i in ins[a:b] if f(i))
    first_mfma = lambda a: next(k for k in range(a, len(ins)) if ins[k][1].startswith('v_mfma'))
    c = dict(
        s1_s3=s3 - s1,
        s1_s3_readlane=n(s1, s3, lambda i: i[1].startswith('v_readlane_b32')),
        s1_s3_branches=n(s1, s3, lambda i: 'branch' in i[1]),
        loop_rcp_iflag=n(head, end + 1, lambda i: i[1].startswith('v_rcp_iflag_f32')),
        s2_s3_div_scale=n(s2, s3, lambda i: i[1].startswith('v_div_scale_f32')),
        publish_stores=n(s1, s2, lambda i: i[1] == 'global_store_dwordx2' and 'sc1' in i[2]),
        poll_loads=polls(ins, s1, s2),
        head_to_forward=first_mfma(head) - head,
        s3_to_backward=first_mfma(s3) - s3 - 1,
        loop=end + 1 - head)
    c.update(metadata(meta, sym) or {})
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('instance', help='"RT, G, PROX, EARLY, TEAMS, WAVES, TPWK, MBK"')
    ap.add_argument('--lib', default=os.path.join(tool.PKG, 'libfedsim.so'))
    o = ap.parse_args()
    sym = tool.mangled(tool.parse_args_str(o.instance))
    listing, meta = tool.disassemble(o.lib, sym)
    for k, v in counts(listing, meta, sym).items():
        print('%-18s %s' % (k, v))
    return 0


if __name__ == '__main__':
    sys.exit(main())
