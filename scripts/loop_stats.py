#!/usr/bin/env python3
"""Static instruction mix of a sweep kernel, basic block by basic block (VALU, broadcast-FMAs, SALU, no-ops, LDS, scratch,
VGPR-index reads): what DESIGN.md's per-trip and per-region tables are counted from.

    cd pink_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -pragma-unroll-threshold=200000 \
        -DPINKHIP_TU_FAMILY=sweep -DPINKHIP_TU_NV=30 -DPINKHIP_TU_MD=0 -DPINKHIP_TU_W=32 --cuda-device-only -S tu_kernel.hip -o /tmp/k.s
    python scripts/loop_stats.py /tmp/k.s

The tableau loop is found from the control-flow graph, not from the compiler's "in Loop" comments (it writes those for
natural loops only, and they pointed at the stacking loop of the hand-over code once the tableau loop was none): it is the
strongly connected component of basic blocks that holds the column read with the VGPR index mode (s_set_gpr_idx_on).
Four reports:

  * the loop, block by block, with each block's successors and the part it is counted in;
  * the ORDINARY TRIP: the blocks of the loop an exchange executes, with its scalar instructions and, among them, its
    conditional branches (issue slots: VALU, SALU and branches count together).  The closing trips are the only part of the loop that
    reads LDS (the stated problem, parked there): blocks that read it, blocks that are only reached through them and
    blocks that only lead to them are left out.  A block that a scalar branch jumps around and that holds none of the
    trip's work (no broadcast-FMA, no index read, no permlane swap, a handful of instructions) is counted as RARE: the
    iteration cap, Murty's rule, the verdict on a pivot of the wrong sign;
  * the INITIAL SWEEPS: the blocks in front of the loop that hold a row's worth of broadcast-FMAs behind one
    bcast_prepare, with the plain 64-bit register moves of each (a row rotated through its registers shows as ~NT / 3 or
    more v_mov_b64), and the vector instructions of the blocks between them: the always-executed tests in front of
    each sweep;
  * the START-UP (the stacking, ik_stack_rows.h): a STACKED ROW is a block in front of the initial sweeps that holds a row's
    worth of broadcast-FMAs and no reciprocal.  Reported: the vector instructions of all blocks between kernel entry and the
    first stacked row, and among them the 64-bit address computations (v_lshl_add_u64, v_mad_u64_u32) and the memory requests;
    the vector instructions per stacked row; and the chunk loop -- the strongly connected component that holds the stacked rows --
    outside its rows: its vector and scalar instructions, its 64-bit address computations and its register-to-register
    v_mov_b64 (a chunk buffer copied into its neighbour; `v_mov_b64 v[..], 0` is a default, not a copy).
"""
import re
import sys

# a block that a scalar branch jumps around is RARE up to this many vector instructions (the cap: 3, Murty's rule: 3, a
# verdict: 4); the selection, which a wave skips only once none of its groups is running, has 18
RARE_MAX = 8
LABEL = re.compile(r'^(\.LBB\d+_\d+):|^; %bb\.(\d+):')


def parse(path):
    lines = [l.rstrip() for l in open(path)]
    ks = [i for i, l in enumerate(lines) if re.match(r'^_ZN7pinkhip\d+ik_solve_sweepx?(_warm)?_kernel.*:', l)][0]
    ke = [i for i in range(ks, len(lines)) if lines[i].strip().startswith('s_endpgm')][0]
    blocks, cur = [], None
    for i in range(ks + 1, ke + 1):
        l = lines[i]
        m = LABEL.match(l)
        if m or cur is None:
            name = (m.group(1) if m.group(1) else 'bb.' + m.group(2)) if m else 'entry'
            cur = dict(name=name, line=i + 1, valu=0, dppf=0, salu=0, cbr=0, nop=0, ds=0, scr=0, idx=0, mov64=0, cp64=0, a64=0, vmem=0, swap=0, ops={}, succ=[], term=False)
            blocks.append(cur)
            if m:
                continue
        s = l.strip()
        if not s or s.startswith(';') or s.startswith('.'):
            continue
        op = s.split()[0]
        if op.startswith('v_'):
            cur['valu'] += 1
            if op == 'v_fmac_f64_dpp':
                cur['dppf'] += 1
            if op.startswith('v_mov_b64') and 'dpp' not in op:
                cur['mov64'] += 1
                if re.match(r'v_mov_b64\S*\s+v\[\d+:\d+\],\s*v\[', s):
                    cur['cp64'] += 1
            if op.startswith(('v_lshl_add_u64', 'v_mad_u64_u32', 'v_mad_i64_i32')):
                cur['a64'] += 1
            if op.startswith('v_permlane'):
                cur['swap'] += 1
        elif op == 's_nop':
            cur['nop'] += 1
        elif op.startswith('ds_'):
            if not op.startswith(('ds_bpermute', 'ds_permute', 'ds_swizzle')):  # (the crossbar: no LDS memory)
                cur['ds'] += 1
        elif op.startswith(('global_load', 'buffer_load', 'flat_load')):
            cur['vmem'] += 1
        elif op.startswith('scratch_'):
            cur['scr'] += 1
        elif op == 's_set_gpr_idx_on':
            cur['idx'] += 1
        elif op.startswith('s_'):
            cur['salu'] += 1
            if op.startswith('s_cbranch'):
                cur['cbr'] += 1
                cur['succ'].append(s.split()[1])
            elif op == 's_branch':
                cur['succ'].append(s.split()[1])
                cur['term'] = True
            elif op == 's_endpgm':
                cur['term'] = True
        cur['ops'][op] = cur['ops'].get(op, 0) + 1
    index = {b['name']: n for n, b in enumerate(blocks)}
    for n, b in enumerate(blocks):
        succ = [index[t] for t in b['succ'] if t in index]
        if not b['term'] and n + 1 < len(blocks):
            succ.append(n + 1)  # falls through
        b['succ'] = sorted(set(succ))
    return blocks


def component_of(blocks, start):
    """the blocks that reach `start` and are reached from it"""
    def reach(adj):
        seen, todo = {start}, [start]
        while todo:
            for t in adj[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return seen
    fwd = [b['succ'] for b in blocks]
    bwd = [[] for _ in blocks]
    for n, b in enumerate(blocks):
        for t in b['succ']:
            bwd[t].append(n)
    return sorted(reach(fwd) & reach(bwd))


def short(name):
    return re.sub(r'^\.LBB\d+_', '', name)


def show(b, blocks, tag=''):
    ops = sorted(((n, o) for o, n in b['ops'].items() if o.startswith('v_') and o != 'v_fmac_f64_dpp'), reverse=True)[:6]
    succ = ','.join(short(blocks[t]['name']) for t in b['succ'])
    print(f"{short(b['name']):8s} L{b['line']:5d} valu {b['valu']:3d} dppfma {b['dppf']:2d} salu {b['salu']:3d} cbr {b['cbr']} nop {b['nop']:2d} ds {b['ds']:2d} "
          f"scr {b['scr']} idx {b['idx']} mov64 {b['mov64']:2d} -> {succ:14s} {tag:8s} {ops}")


def main():
    blocks = parse(sys.argv[1])
    idx_blocks = [n for n, b in enumerate(blocks) if b['idx']]
    if not idx_blocks:
        sys.exit("no VGPR-index read in this kernel: not an instantiation with the indexed column")
    loop = component_of(blocks, idx_blocks[0])
    inloop, header = set(loop), loop[0]
    print(f"tableau loop: {len(loop)} blocks, lines {blocks[loop[0]]['line']} .. {blocks[loop[-1]]['line']}, "
          f"{sum(blocks[n]['dppf'] for n in loop)} broadcast-FMAs, {sum(blocks[n]['valu'] for n in loop)} VALU on all paths")
    work = lambda n: blocks[n]['idx'] or blocks[n]['dppf'] >= 8 and not blocks[n]['ds']  # noqa: E731  (the trip's own work)
    preds = {n: [p for p in loop if n in blocks[p]['succ'] and p != n] for n in loop}
    closing = {n for n in loop if blocks[n]['ds']}
    changed = True
    while changed:
        changed = False
        for n in loop:
            if n in closing or n == header:
                continue
            ss = [t for t in blocks[n]['succ'] if t in inloop and t != n]
            if (preds[n] and all(p in closing for p in preds[n])) or (not work(n) and ss and all(t in closing for t in ss)):
                closing.add(n)
                changed = True
    rare, trip = [], []
    for n in loop:
        b = blocks[n]
        if n in closing:
            continue
        ps = [p for p in preds[n] if p not in closing]
        around = len(ps) == 1 and len(b['succ']) == 1 and b['succ'][0] in blocks[ps[0]]['succ'] and not work(n) and not b['swap'] and not b['dppf'] and b['valu'] <= RARE_MAX
        (rare if around else trip).append(n)
    print("\n-- the loop, block by block")
    for n in loop:
        show(blocks[n], blocks, 'closing' if n in closing else ('rare' if n in rare else 'trip'))
    t = [blocks[n] for n in trip]
    print(f"\nORDINARY TRIP: {sum(b['valu'] for b in t)} VALU, of which {sum(b['dppf'] for b in t)} broadcast-FMAs and "
          f"{sum(b['mov64'] for b in t)} v_mov_b64; {sum(b['salu'] for b in t)} SALU, of which {sum(b['cbr'] for b in t)} conditional branches; "
          f"{sum(b['nop'] for b in t)} s_nop, {sum(b['scr'] for b in t)} scratch")
    print(f"  behind scalar branches a trip jumps around (RARE): {sum(blocks[n]['valu'] for n in rare)} VALU, {sum(blocks[n]['salu'] for n in rare)} SALU "
          f"in {len(rare)} blocks")
    print(f"  closing trips only: {sum(blocks[n]['valu'] for n in closing)} VALU, {sum(blocks[n]['salu'] for n in closing)} SALU in {len(closing)} blocks")
    # the closing trips in a loop of their own (PINKHIP_SWEEP_SPLIT_CLOSING): the first loop behind the tableau loop that reads
    # LDS and holds a row's worth of broadcast-FMAs
    if not closing:
        for n in range(loop[-1] + 1, len(blocks)):
            if blocks[n]['ds'] and n not in inloop:
                comp = component_of(blocks, n)
                if len(comp) > 1 and sum(blocks[m]['dppf'] for m in comp) >= 8:
                    c = [blocks[m] for m in comp]
                    print(f"  CLOSING LOOP (separate): {len(comp)} blocks, lines {c[0]['line']} .. {c[-1]['line']}: {sum(b['valu'] for b in c)} VALU, "
                          f"{sum(b['dppf'] for b in c)} broadcast-FMAs, {sum(b['mov64'] for b in c)} v_mov_b64, {sum(b['salu'] for b in c)} SALU, "
                          f"{sum(b['scr'] for b in c)} scratch on all paths")
                    break
    mix = {}
    for b in t:
        for o, c in b['ops'].items():
            if o.startswith('v_'):
                mix[o] = mix.get(o, 0) + c
    print("  trip mix:", ', '.join(f"{o} {c}" for o, c in sorted(mix.items(), key=lambda x: -x[1])))
    # ---- initial sweeps: blocks in front of the loop with a row's worth of broadcast-FMAs behind one bcast_prepare
    # (... and the reciprocal of its pivot: what tells a sweep from a chunk of the stacking and from the start product)
    front = [n for n in range(loop[0]) if blocks[n]['dppf'] >= 12 and 1 <= blocks[n]['swap'] <= 8 and blocks[n]['valu'] <= 3 * blocks[n]['dppf'] + 10
             and not blocks[n]['ds'] and blocks[n]['ops'].get('v_rcp_f64_e32')]
    if front:
        print("\n-- initial sweeps")
        first, last = front[0], front[-1]
        between = [n for n in range(first, last + 1) if n not in front]
        rot = lambda n: blocks[n]['mov64'] >= 6  # noqa: E731
        for n in front:
            show(blocks[n], blocks, 'ROW MOVES' if rot(n) else '')
        vs = [blocks[n]['valu'] for n in front]
        print(f"INITIAL SWEEPS: {len(front)} blocks, VALU min {min(vs)} max {max(vs)}, blocks with row moves: {sum(1 for n in front if rot(n))}")
        print(f"  always-executed code between them: {sum(blocks[n]['valu'] for n in between)} VALU in {len(between)} blocks")
        n = first - 1
        while n > 0 and blocks[n]['valu'] == 0:
            n -= 1
        show(blocks[n], blocks, 'in front')
        startup(blocks, front[0])


def startup(blocks, first_sweep):
    rows = [n for n in range(first_sweep) if blocks[n]['dppf'] >= 12 and blocks[n]['swap'] and not blocks[n]['ops'].get('v_rcp_f64_e32')]
    if not rows:
        return
    print("\n-- start-up (stacking)")
    head = blocks[:rows[0]]
    print(f"ENTRY TO FIRST STACKED ROW: {sum(b['valu'] for b in head)} VALU, of which {sum(b['a64'] for b in head)} 64-bit address computations; "
          f"{sum(b['salu'] for b in head)} SALU, of which {sum(b['cbr'] for b in head)} conditional branches; {sum(b['vmem'] for b in head)} memory requests, "
          f"in {len(head)} blocks (all paths)")
    vs = [blocks[n]['valu'] for n in rows]
    print(f"STACKED ROWS: {len(rows)} blocks, VALU min {min(vs)} max {max(vs)}, broadcast-FMAs {blocks[rows[0]]['dppf']}, SALU min "
          f"{min(blocks[n]['salu'] for n in rows)} max {max(blocks[n]['salu'] for n in rows)}")
    comp = component_of(blocks, rows[0])
    rest = [blocks[n] for n in comp if n not in rows]
    print(f"CHUNK LOOP: {len(comp)} blocks of which {sum(1 for n in comp if n in rows)} stacked rows; outside the rows: {sum(b['valu'] for b in rest)} VALU, "
          f"of which {sum(b['cp64'] for b in rest)} register-to-register v_mov_b64 and {sum(b['a64'] for b in rest)} 64-bit address computations; "
          f"{sum(b['salu'] for b in rest)} SALU, of which {sum(b['cbr'] for b in rest)} conditional branches; {sum(b['vmem'] for b in rest)} memory requests")


if __name__ == '__main__':
    main()
