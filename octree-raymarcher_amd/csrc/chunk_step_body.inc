// chunk_step_body.inc — the body of the hand-scheduled chunk step; included by chunk_step_asm.hip.h once per variant, each time the
// specialization ChunkStepAsm<SVO_CHUNK_BIG, SVO_CHUNK_GLSL, SVO_CHUNK_SEG> (SVO_CHUNK_WIDE_BASE: how wide_b is formed;
// SVO_CHUNK_ESCAPE_GUARD: the shader's guard; SVO_CHUNK_FAR_END: the bounded rays' far end).  See chunk_step_asm.hip.h for the commentary.
#ifndef SVO_CHUNK_ESCAPE
// escape(a, g, clo, clo + csize) of march.hip.h into q1, a = (AX, AY, AZ): t0 = (lo - a) * g, t1 = (hi - a) * g, per axis
// gmax(t0, t1) = (t0 < t1) ? t1 : t0, then gmin(tx, gmin(ty, tz)) with gmin(x, y) = (y < x) ? y : x.  FILL: exactly one
// instruction that touches neither q2, q3 nor VCC - with the s_nop 0 behind it the two wait states between that v_cmp and its v_cndmask;
// a caller with nothing to do there passes "s_nop 0".
#define SVO_CHUNK_ESCAPE(AX, AY, AZ, FILL) \
        "v_add_f32 %[h1], %[csz], %[clx]\n\t" \
        "v_add_f32 %[h2], %[csz], %[cly]\n\t" \
        "v_add_f32 %[h3], %[csz], %[clz]\n\t" \
        "v_sub_f32 %[q1], %[clx], %[" AX "]\n\t" \
        "v_sub_f32 %[q2], %[cly], %[" AY "]\n\t" \
        "v_sub_f32 %[q3], %[clz], %[" AZ "]\n\t" \
        "v_sub_f32 %[q4], %[h1], %[" AX "]\n\t" \
        "v_sub_f32 %[q5], %[h2], %[" AY "]\n\t" \
        "v_sub_f32 %[q6], %[h3], %[" AZ "]\n\t" \
        "v_mul_f32 %[q1], %[q1], %[gx]\n\t" \
        "v_mul_f32 %[q2], %[q2], %[gy]\n\t" \
        "v_mul_f32 %[q3], %[q3], %[gz]\n\t" \
        "v_mul_f32 %[q4], %[q4], %[gx]\n\t" \
        "v_mul_f32 %[q5], %[q5], %[gy]\n\t" \
        "v_mul_f32 %[q6], %[q6], %[gz]\n\t" \
        "v_cmp_lt_f32 vcc, %[q1], %[q4]\n\t" \
        "v_cmp_lt_f32_e64 %[ss1], %[q2], %[q5]\n\t" \
        "v_cmp_lt_f32_e64 %[ss2], %[q3], %[q6]\n\t" \
        "v_cndmask_b32 %[q1], %[q1], %[q4], vcc\n\t" \
        "v_cndmask_b32_e64 %[q2], %[q2], %[q5], %[ss1]\n\t" \
        "v_cndmask_b32_e64 %[q3], %[q3], %[q6], %[ss2]\n\t" \
        "v_cmp_lt_f32 vcc, %[q3], %[q2]\n\t" \
        FILL \
        "s_nop 0\n\t" \
        "v_cndmask_b32 %[q2], %[q2], %[q3], vcc\n\t" \
        "v_cmp_lt_f32 vcc, %[q2], %[q1]\n\t" \
        "s_nop 1\n\t" \
        "v_cndmask_b32 %[q1], %[q1], %[q2], vcc\n\t"
#endif

template <>
struct ChunkStepAsm<SVO_CHUNK_BIG, SVO_CHUNK_GLSL, SVO_CHUNK_SEG> {
template <int TAB>
static __device__ __forceinline__ unsigned long long run(
    int &mode, float &tw, int &cw, int &ci, int &valid, int &pux, int &puy, int &puz, V3 &clo, WideRef<SVO_CHUNK_BIG> &wide_b,
    uint32_t &twig_off, int &levels, V3 &O, float &t, int &cnt, V3 &Blo, float &res, float &bsize, float &res_tree, int &nw,
    const V3 alpha, const V3 beta, const V3 g, [[maybe_unused]] const float far,
    const float Ginv, const int Goff0, const int Goff1, const int Goff2, const int Gdimw, const int Gdimh, const int Gdimd,
    const uint32_t table_in_lds, const uint32_t lds_tab, const ChunkStepUniform U)
{
    float h1, h2, h3, q1, q2, q3, q4, q5, q6;                  // the chunk box's far corner; scratch (once the chunk index exists in q4:
    unsigned long long sall, sw, smiss, ss1, ss2;               // q5 the table address, q3 / q6 / q2 the entry's levels, wide_off, twig_off)
    asm volatile(
        "s_mov_b64 %[sall], exec\n\t"
        "s_mov_b64 %[smiss], 0\n\t"
        "v_cmpx_eq_u32 vcc, 1, %[md]\n\t"                       // the lanes in M_WORLD
        "s_cbranch_execz 9f\n\t"
        "s_mov_b64 %[sw], exec\n\t"
        // ---- left its chunk in the step (cw's top bit): tw += escape(O, g, chunk box) + EPS, src/Traverse.cpp:164-168
        "v_cmpx_gt_i32 vcc, 0, %[cw]\n\t"
        "s_cbranch_execz 1f\n\t"
        SVO_CHUNK_ESCAPE("ox", "oy", "oz", "v_and_b32 %[cw], 0x7fffffff, %[cw]\n\t")
        SVO_CHUNK_ESCAPE_GUARD
        "v_add_f32 %[q1], %[eps], %[q1]\n\t"
        "v_add_f32 %[tw], %[tw], %[q1]\n\t"
        "1:\n\t"
        "s_mov_b64 exec, %[sw]\n\t"
        // ---- the chunk cap (:142) and the far end; EXEC narrows to the rays that go on, what falls out of it is the miss mask
        "v_cmpx_gt_i32 vcc, %[capc], %[cw]\n\t"
        SVO_CHUNK_FAR_END
        "v_add_u32 %[cw], 1, %[cw]\n\t"
        // ---- p = alpha + beta * tw (:144) inside the world box (:145), closed, a NaN fails.  p is formed in O, where treemarch wants it
        //      (a = p, :158): no lane in M_WORLD reads O once its pending escape is taken - a ray that ends here or steps on in M_WORLD
        //      never looks at it again, the next chunk it enters writes it
        "v_mul_f32 %[ox], %[bx], %[tw]\n\t"
        "v_mul_f32 %[oy], %[by], %[tw]\n\t"
        "v_mul_f32 %[oz], %[bz], %[tw]\n\t"
        "v_add_f32 %[ox], %[ax], %[ox]\n\t"
        "v_add_f32 %[oy], %[ay], %[oy]\n\t"
        "v_add_f32 %[oz], %[az], %[oz]\n\t"
        "v_cmpx_le_f32 vcc, %[wlx], %[ox]\n\t"
        "v_cmpx_le_f32 vcc, %[wly], %[oy]\n\t"
        "v_cmpx_le_f32 vcc, %[wlz], %[oz]\n\t"
        "v_cmpx_ge_f32 vcc, %[whx], %[ox]\n\t"
        "v_cmpx_ge_f32 vcc, %[why], %[oy]\n\t"
        "v_cmpx_ge_f32 vcc, %[whz], %[oz]\n\t"
        "s_andn2_b64 %[smiss], %[sw], exec\n\t"
        "s_cbranch_execz 9f\n\t"
        // ---- World::index_float(p) as the grid cell (chunk_cell_pow2) and World::index of it (chunk_index_u24)
        "v_mul_f32 %[q1], %[ox], %[ginv]\n\t"
        "v_mul_f32 %[q2], %[oy], %[ginv]\n\t"
        "v_mul_f32 %[q3], %[oz], %[ginv]\n\t"
        "v_cmp_gt_f32 vcc, 0, %[q1]\n\t"
        "v_cmp_gt_f32_e64 %[ss1], 0, %[q2]\n\t"
        "v_cmp_gt_f32_e64 %[ss2], 0, %[q3]\n\t"
        "v_add_f32 %[q4], -1.0, %[q1]\n\t"
        "v_add_f32 %[q5], -1.0, %[q2]\n\t"
        "v_add_f32 %[q6], -1.0, %[q3]\n\t"
        "v_cndmask_b32 %[q1], %[q1], %[q4], vcc\n\t"
        "v_cndmask_b32_e64 %[q2], %[q2], %[q5], %[ss1]\n\t"
        "v_cndmask_b32_e64 %[q3], %[q3], %[q6], %[ss2]\n\t"
        "v_cvt_i32_f32 %[q1], %[q1]\n\t"
        "v_cvt_i32_f32 %[q2], %[q2]\n\t"
        "v_cvt_i32_f32 %[q3], %[q3]\n\t"
        "v_add_u32 %[q1], %[q1], %[gox]\n\t"
        "v_add_u32 %[q2], %[q2], %[goy]\n\t"
        "v_add_u32 %[q3], %[q3], %[goz]\n\t"
        "v_add_u32 %[q4], %[q1], %[gdw]\n\t"                    // wrap_once: of m, m + dim, m - dim the one in [0, dim) is the smallest unsigned
        "v_add_u32 %[q5], %[q2], %[gdh]\n\t"
        "v_add_u32 %[q6], %[q3], %[gdd]\n\t"
        "v_sub_u32 %[h1], %[q1], %[gdw]\n\t"
        "v_sub_u32 %[h2], %[q2], %[gdh]\n\t"
        "v_sub_u32 %[h3], %[q3], %[gdd]\n\t"
        "v_min3_u32 %[q1], %[q1], %[q4], %[h1]\n\t"
        "v_min3_u32 %[q2], %[q2], %[q5], %[h2]\n\t"
        "v_min3_u32 %[q3], %[q3], %[q6], %[h3]\n\t"
        "v_mad_u32_u24 %[q4], %[q2], %[gdd], %[q3]\n\t"          // (my * dimd + mz) * dimw + mx
        "v_mad_u32_u24 %[q4], %[q4], %[gdw], %[q1]\n\t"
        "v_cmp_ne_u32_e64 %[ss1], %[q4], %[ci]\n\t"             // another chunk: nothing of the descent cache holds
        // ---- the chunk's table entry: bmin, levels, wide_off, twig_off
        "s_cmp_lg_u32 %[tinl], 0\n\t"
        "s_cbranch_scc0 5f\n\t"
        "v_lshl_add_u32 %[q5], %[q4], 2, %[tab]\n\t"
        "ds_read_b32 %[clx], %[q5]\n\t"
        "ds_read_b32 %[cly], %[q5] offset:%[t1]\n\t"
        "ds_read_b32 %[clz], %[q5] offset:%[t2]\n\t"
        "ds_read_b32 %[q3], %[q5] offset:%[t3]\n\t"
        "ds_read_b32 %[q6], %[q5] offset:%[t4]\n\t"
        "ds_read_b32 %[q2], %[q5] offset:%[t5]\n\t"
        "6:\n\t"
        "v_cndmask_b32_e64 %[val], %[val], 0, %[ss1]\n\t"
        "v_cndmask_b32_e64 %[pux], %[pux], 0, %[ss1]\n\t"
        "v_cndmask_b32_e64 %[puy], %[puy], 0, %[ss1]\n\t"
        "v_cndmask_b32_e64 %[puz], %[puz], 0, %[ss1]\n\t"
        "v_mov_b32 %[ci], %[q4]\n\t"
        "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t"
        // ---- isInsideCube(p, bmin, bmin + chunksize), src/Traverse.cpp:154-155
        "v_add_f32 %[h1], %[csz], %[clx]\n\t"
        "v_add_f32 %[h2], %[csz], %[cly]\n\t"
        "v_add_f32 %[h3], %[csz], %[clz]\n\t"
#if SVO_CHUNK_GLSL
        "s_mov_b64 %[ss2], exec\n\t"
#endif
        "v_cmpx_ge_f32 vcc, %[ox], %[clx]\n\t"
        "v_cmpx_ge_f32 vcc, %[oy], %[cly]\n\t"
        "v_cmpx_ge_f32 vcc, %[oz], %[clz]\n\t"
        "v_cmpx_ge_f32 vcc, %[h1], %[ox]\n\t"
        "v_cmpx_ge_f32 vcc, %[h2], %[oy]\n\t"
        "v_cmpx_ge_f32 vcc, %[h3], %[oz]\n\t"
#if SVO_CHUNK_GLSL
        "s_andn2_b64 %[ss2], %[ss2], exec\n\t"                  // not contained: the shader steps on out of that box (below)
#else
        "s_andn2_b64 %[smiss], %[sw], exec\n\t"                 // not contained: the ray ends
#endif
        "s_cbranch_execz 8f\n\t"
        // ---- contained: treemarch(p, beta, chunk), a = p, t = 0 (src/Traverse.cpp:158,78) - the tree level's frame
        SVO_CHUNK_WIDE_BASE
        "v_mov_b32 %[tof], %[q2]\n\t"
        "v_mov_b32 %[lev], %[q3]\n\t"
        "v_sub_u32 %[rs], 127, %[q3]\n\t"
        "v_add_u32 %[nw], 1, %[q3]\n\t"
        "v_lshlrev_b32 %[rs], 23, %[rs]\n\t"                    // 2^-levels
        "v_lshrrev_b32 %[nw], 1, %[nw]\n\t"
        "v_mov_b32 %[t], 0\n\t"
        "v_mov_b32 %[cnt], %[capt]\n\t"
        "v_mov_b32 %[lx], %[clx]\n\t"
        "v_mov_b32 %[ly], %[cly]\n\t"
        "v_mov_b32 %[lz], %[clz]\n\t"
        "v_mul_f32 %[rs], %[csz], %[rs]\n\t"                    // csize / 2^levels, exact
        "v_mov_b32 %[bs], %[csz]\n\t"
        "v_max_u32 %[nw], 1, %[nw]\n\t"                         // levels ? (levels + 1) >> 1 : 1
        "v_mov_b32 %[rtr], %[rs]\n\t"
        "v_mov_b32 %[md], 3\n\t"
        "8:\n\t"
#if SVO_CHUNK_GLSL
        "s_mov_b64 exec, %[ss2]\n\t"
        "s_cbranch_execz 9f\n\t"
        SVO_CHUNK_ESCAPE("ox", "oy", "oz", "s_nop 0\n\t")
        SVO_CHUNK_ESCAPE_GUARD
        "v_add_f32 %[q1], %[eps], %[q1]\n\t"
        "v_add_f32 %[tw], %[tw], %[q1]\n\t"                     // (stays M_WORLD; cw counts it)
#endif
        "s_branch 9f\n\t"
        // ---- out of line: the table lies in A.wchunks (more chunks than the LDS table holds)
        "5:\n\t"
        "s_load_dwordx2 %[ss2], %[karg], %[wchoff]\n\t"          // TraceArgs::wchunks
        "v_lshlrev_b32 %[q5], 5, %[q4]\n\t"                     // 32-byte entries, fewer than 2^24 of them
        "s_waitcnt lgkmcnt(0)\n\t"
        "global_load_dword %[clx], %[q5], %[ss2]\n\t"
        "global_load_dword %[cly], %[q5], %[ss2] offset:4\n\t"
        "global_load_dword %[clz], %[q5], %[ss2] offset:8\n\t"
        "global_load_dword %[q3], %[q5], %[ss2] offset:12\n\t"
        "global_load_dword %[q6], %[q5], %[ss2] offset:16\n\t"
        "global_load_dword %[q2], %[q5], %[ss2] offset:24\n\t"
        "s_branch 6b\n\t"
        "9:\n\t"
        "s_mov_b64 exec, %[sall]\n\t"
        : [md] "+v"(mode), [tw] "+v"(tw), [cw] "+v"(cw), [ci] "+v"(ci), [val] "+v"(valid), [pux] "+v"(pux), [puy] "+v"(puy), [puz] "+v"(puz),
          [clx] "+v"(clo.x), [cly] "+v"(clo.y), [clz] "+v"(clo.z), [wb] "+v"(wide_b), [tof] "+v"(twig_off), [lev] "+v"(levels),
          [ox] "+v"(O.x), [oy] "+v"(O.y), [oz] "+v"(O.z), [t] "+v"(t), [cnt] "+v"(cnt), [lx] "+v"(Blo.x), [ly] "+v"(Blo.y), [lz] "+v"(Blo.z),
          [rs] "+v"(res), [bs] "+v"(bsize), [rtr] "+v"(res_tree), [nw] "+v"(nw),
          [h1] "=&v"(h1), [h2] "=&v"(h2), [h3] "=&v"(h3),
          [q1] "=&v"(q1), [q2] "=&v"(q2), [q3] "=&v"(q3), [q4] "=&v"(q4), [q5] "=&v"(q5), [q6] "=&v"(q6),
          [sall] "=&s"(sall), [sw] "=&s"(sw), [smiss] "=&s"(smiss), [ss1] "=&s"(ss1), [ss2] "=&s"(ss2)
        : [ax] "v"(alpha.x), [ay] "v"(alpha.y), [az] "v"(alpha.z), [bx] "v"(beta.x), [by] "v"(beta.y), [bz] "v"(beta.z),
          [gx] "v"(g.x), [gy] "v"(g.y), [gz] "v"(g.z),
#if SVO_CHUNK_SEG
          [far] "v"(far),
#endif
          [ginv] "v"(Ginv), [gox] "v"(Goff0), [goy] "v"(Goff1), [goz] "v"(Goff2), [gdw] "v"(Gdimw), [gdh] "v"(Gdimh), [gdd] "v"(Gdimd),
          [tab] "s"(lds_tab), [tinl] "s"(table_in_lds),
          [wlx] "s"(U.wlo.x), [wly] "s"(U.wlo.y), [wlz] "s"(U.wlo.z), [whx] "s"(U.whi.x), [why] "s"(U.whi.y), [whz] "s"(U.whi.z),
          [csz] "s"(U.csize), [eps] "s"(U.eps), [capc] "s"(U.cap_chunk), [capt] "s"(U.cap_tree), [karg] "s"(U.kernarg),
#if SVO_CHUNK_BIG
          [widep] "s"(U.wide),
#endif
          [t1] "n"(TAB * 4), [t2] "n"(TAB * 8), [t3] "n"(TAB * 12), [t4] "n"(TAB * 16), [t5] "n"(TAB * 20),
          [wchoff] "n"(__builtin_offsetof(TraceArgs, wchunks))
        : "vcc", "scc", "memory");
    return smiss;
}
};

