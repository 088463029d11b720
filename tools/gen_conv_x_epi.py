#!/usr/bin/env python3
"""Generator of k_conv_x.hip's tile epilogue as ONE `asm volatile` statement per ring stage  ->  disco_diffdock_amd/csrc/k_conv_x_epi_gen.inc   (round 5)

k_conv_x.hip alternates the two waves of a SIMD: one bursts 28 MFMAs while its partner runs the VALU epilogue of its tile; the tile period is the wave-serial
chain burst + epilogue + barrier, and the compiler's epilogue carries ~40 instructions that are not the algorithm's (23-27 v_mov at the merge of the fast and
the slow path, v_cndmask / v_cmp pairs, conservative lgkmcnt(0) waits: VERDICT r04 #1a).  This statement is the whole epilogue - bias, ring stores, fold,
tile kind, packed quad, flush - with the accumulators as in/out operands, D0 / D1 / f0 in pinned registers (element access) and scalar branches inside, so every
tile kind works on the same registers.  The instruction streams are tools/gen_conv_y.py's (same arithmetic, same order as the C++ epilogue it replaces;
reference models/tensor_layers.py:65-116,147-159)."""
import os
import gen_conv_y as G

TB, LIMB = 13968, 4608
BIAS_OFF = 3 * LIMB
# registers: D0 = v[16:31] (in/out: folded in place), D1 = v[32:47], f0 = v[48:51]; scratch v0..v15 (bias; then f1 v0-3, f2 v4-7, g0 v8-11, R v12-15; flush values v0-8,
# w = v / sqrt2 in v9-11), v52 packed-quad sum / g0 address, v53 flush address
G.DBASE['x'] = 16
G._Y[0] = 'x'
G.B[:] = [f'v{i}' for i in range(16)]
F0 = [f'v{48 + i}' for i in range(4)]
G.F = F0 + [f'v{i}' for i in range(12)]
G.FQ[:] = [f'v{i}' for i in range(9)]
G.FO = 'v53'
G.XQ = 'v52'
R = ['v12', 'v13', 'v14', 'v15']
CLOBBER = [f'v{i}' for i in range(16)] + ['v52', 'v53']


def fix(lines):
    out = []
    for ln in lines:
        if isinstance(ln, tuple):
            continue          # ('need', ...) markers: the waits are placed by hand below
        for k in range(4):
            ln = ln.replace(f'%[R{k}]', R[k])
        ln = ln.replace('%[pchan]', '%[chan4]')      # (gen_conv_y's name of the column offset operand)
        out.append(ln)
    return out


def flush(mode, rts):
    G.FO, G.XQ = 'v53', 'v52'
    lines = fix(G.flush_stream(mode))
    if mode == 'S':
        res = []
        for ln in lines:
            if ln.startswith('v_mov_b32 v1') and ln.endswith(', 0') and ln.split()[1].rstrip(',') in R:
                continue                                              # (R is scratch here: no reset)
            if not rts:
                for k in range(4):
                    ln = ln.replace(f'v_mov_b32 %[aV{k}0], {R[k]}', f'v_mov_b32 %[aV{k}0], 0')
            res.append(ln)
        return res
    pre = ['v_mul_f32 v9, 0x3f3504f3, %[vx]', 'v_mul_f32 v10, 0x3f3504f3, %[vy]', 'v_mul_f32 v11, 0x3f3504f3, %[vz]']
    return pre + [ln.replace('%[wx]', 'v9').replace('%[wy]', 'v10').replace('%[wz]', 'v11') for ln in lines]


def kind_body(kind):
    body = []
    if kind.startswith('TV'):
        body += [f'ds_read_b128 v[0:3], %[fpa] offset:16', f'ds_read_b128 v[4:7], %[fpa] offset:32']
        ms = G.main_stream(kind, packed=False)
        out, seen = [], 0
        for it in ms:
            if isinstance(it, tuple):
                if it[1] == 'f1':
                    out.append('s_waitcnt lgkmcnt(1)')
                elif it[1] == 'f2':
                    out.append('s_waitcnt lgkmcnt(0)')
                continue
            out.append(it)
        return body + fix(out)
    return fix(G.main_stream(kind, packed=False))


def epilogue(ST):
    SO, SW = ST * TB, ((ST + 3) & 3) * TB
    L = []
    for j in range(4):
        L.append(f'ds_read_b128 v[{4 * j}:{4 * j + 3}], %[ringb] offset:{SO + BIAS_OFF + 16 * j}')
    # this thread's two chunks of record t+3 (requested at the start of the burst) into the stage tile t-1 has left
    L += ['s_waitcnt vmcnt(1)', f'ds_write_b128 %[rw0], %[st0] offset:{SW}', 's_waitcnt vmcnt(0)', f'ds_write_b128 %[rw1], %[st1] offset:{SW}']
    if not os.environ.get('GEN_ONE_ACC'):      # (the two-limb form has one accumulator chain: nothing to fold)
        for r in range(16):
            L.append(f'v_add_f32 v{16 + r}, v{16 + r}, v{32 + r}')
    L.append('s_waitcnt lgkmcnt(2)')      # the bias reads; the two ring stores stay in flight
    for r in range(16):
        L.append(f'v_fmac_f32 v{16 + r}, v{r}, %[bsc2]')
    # tile kind -> selector (1 RA, 2 RT, 3 + cross bits TV, 7 RTS)
    L += ['s_and_b32 %[t0], %[w0], 3', 's_bfe_u32 %[t1], %[w0], 0x2000e', 's_add_i32 %[t1], %[t1], 3', 's_add_i32 %[t2], %[t0], 1',
          's_cmp_eq_u32 %[t0], 2', 's_cselect_b32 %[t2], %[t1], %[t2]', 's_cmp_eq_u32 %[t0], 3', 's_cselect_b32 %[sel], 7, %[t2]']
    variants = [(1, kind_body('RA')), (2, kind_body('RT'))] + [(3 + x, kind_body(f'TV{x}')) for x in range(4)] + [(7, kind_body('RTS'))]
    inl, ool_k = G.dispatch_split(variants, 'sel', 'k')
    L += inl
    # packed quad (6-channel columns: accumulator quad 3 carries another a / c row quad for channel pair xp)
    L += ['s_bitcmp0_b32 %[w0], 7', 's_cbranch_scc1 .Lnp_%=',
          's_lshr_b32 %[t0], %[w0], 6', 's_and_b32 %[t0], %[t0], 0xf0', 'v_add_u32 v52, %[t0], %[fra]', 'ds_read_b128 v[8:11], v52',
          's_bfe_u32 %[t1], %[w0], 0x20008',
          's_cmp_eq_u32 %[t1], 0', 's_cselect_b32 %[pk0], 1.0, 0', 's_cmp_eq_u32 %[t1], 1', 's_cselect_b32 %[pk1], 1.0, 0', 's_cmp_eq_u32 %[t1], 2', 's_cselect_b32 %[pk2], 1.0, 0',
          's_waitcnt lgkmcnt(0)']
    L += fix([it for it in G.packed_stream() if not isinstance(it, tuple)])
    L.append('.Lnp_%=:')
    # flush of the column this tile closes
    L += ['s_bfe_u32 %[t0], %[w0], 0x20002', 's_cmp_eq_u32 %[t0], 0', 's_cbranch_scc1 .Lnf_%=', 's_cmp_eq_u32 %[t0], 2', 's_cbranch_scc1 .Lfv_%=',
          's_cmp_eq_u32 %[sel], 7', 's_cbranch_scc1 .Lfr_%=']
    L += flush('S', False) + ['s_branch .Lnf_%=', '.Lfr_%=:'] + flush('S', True) + ['s_branch .Lnf_%=', '.Lfv_%=:'] + flush('V', False)
    L += ['.Lnf_%=:', 's_waitcnt lgkmcnt(0)', 's_branch .Lexit_%='] + ool_k + ['.Lexit_%=:']
    return L


def main():
    out = ['// GENERATED by tools/gen_conv_x_epi.py - do not edit.\n']
    accs = [o for o in G.acc_ops('') if not o[0].startswith('R')]
    outs = [('D0', '+{v[16:31]}', 'D0')] + accs + [(n, '=&s', f'{n}_') for n in ('t0', 't1', 't2', 'sel', 'pk0', 'pk1', 'pk2', 'sv')]
    one_acc = bool(os.environ.get('GEN_ONE_ACC'))      # one accumulator chain (the two-limb form, k_conv_x.hip X3_TWO_LIMBS -> k_conv_x2.hip): no D1 operand, nothing to fold
    ins = ([] if one_acc else [('D1', '{v[32:47]}', 'D1')]) + [('f0', '{v[48:51]}', 'f0'), ('st0', 'v', 'st0'), ('st1', 'v', 'st1'), ('ringb', 'v', 'ringb_u'), ('rw0', 'v', 'ringw0_u'),
           ('rw1', 'v', 'ringw1_u'), ('fpa', 'v', 'fpa_u'), ('fra', 'v', 'fra_u'), ('bsc2', 'v', 'bsc2'), ('oscv', 'v', 'oscv'), ('s0', 'v', 's0'), ('vx', 'v', 'vx'),
           ('vy', 'v', 'vy'), ('vz', 'v', 'vz'), ('sm1', 'v', 'seg.m1'), ('sm2', 'v', 'seg.m2'), ('sm4', 'v', 'seg.m4'), ('sm8', 'v', 'seg.m8'), ('sm16', 'v', 'seg.m16'),
           ('vrow', 'v', 'vrow'), ('hh4', 'v', 'hh4_u'), ('hh12', 'v', 'hh12_u'), ('w0', 's', 'w0'), ('chan4', 's', 'chan4_'), ('tail', 's', 'tail_mask'),
           ('sumbase', 's', 'sumbase')]
    for ST in range(4):
        lines = epilogue(ST)
        txt = G.asm_stmt(f'X3_EPI_{ST}', lines, outs, ins, CLOBBER + ['memory', 'scc'])
        out.append(txt)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'disco_diffdock_amd', 'csrc', os.environ.get('GEN_OUT', 'k_conv_x_epi_gen.inc'))
    with open(path, 'w') as f:
        f.write('\n'.join(out))
    print('wrote', os.path.normpath(path), sum(s.count('\n') for s in out), 'lines')


if __name__ == '__main__':
    main()
