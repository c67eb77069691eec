// chunk_step_asm.hip.h — the chunk step of k_trace_stack (src/Traverse.cpp:142-168), hand-scheduled for gfx950 (one asm statement).
//
// Same arithmetic, operand for operand and in the same order, as the C++ twin in chunk_step_cxx.hip.h (`if (mode == M_WORLD)`, which
// stays the readable statement of the algorithm and the A/B partner: -DSVO_CXX_STEP builds it); what differs is what the compiler
// puts around it - a s_and_saveexec / s_or pair per source-level `if` (six of them nested), three box tests whose six compares are
// and-ed through scalar chains, and 23 lane registers copied at the joins.  Here, in the idiom of step_asm.hip.h:
//   * the lanes in M_WORLD, the pending escape, the chunk cap, the world box and the chunk's own box narrow EXEC directly (v_cmpx
//     chains, a world-box bound being the one SGPR operand an instruction may have); EXEC is put back once, at the end;
//   * every outcome class (pending escape / past the cap / inside the world / contained) is entered by one EXEC write and writes the
//     lane state in place: nothing is copied at a join, and this statement is the ONLY place that writes the chunk's lane registers;
//   * the six words of the chunk's table entry are requested as soon as the chunk index exists and waited for behind the descent
//     cache's reset; "table in LDS" / "table in A.wchunks" is a wave-uniform scalar branch inside the statement (the large table: the
//     pointer is read from the kernarg segment where it is needed, then six vector loads at a 32-bit offset from it);
//   * escape() keeps its literal compare-and-select form (glm's min / max order NaN differently from v_max / v_min3), p = alpha +
//     beta * tw is a multiply and an add, the chunk cell is product, `q < 0 -> q - 1`, truncation, + off, wrap_once (add, subtract,
//     v_min3_u32), the index two v_mad_u32_u24;
//   * p is formed in O, where treemarch wants it: O is dead for a lane in M_WORLD once its pending escape is taken (chunk_step_body.inc).
// The statement writes no memory: the lanes that miss (cap, far end, world box, containment) come back as a mask, and the kernel
// stores their records behind it.  The chunk grid's eight words are read from LDS by the caller (two 16-byte reads at a uniform
// address, which an asm operand cannot take apart) and handed in as lane values.
//
// Hazards honoured by hand: v_cmp writing VCC / an SGPR pair -> v_cndmask reading it: two instructions in between; every LDS read and
// load is waited for before its first use, so every output is valid when the statement ends.
//
// Variants, fragments of the one text (chunk_step_body.inc is included once per variant):
//   BIG   wide_b is a 64-bit address (wide pool base + wide_off * 256, one v_mad_u64_u32) instead of a 32-bit byte offset;
//   GLSL  the guarded escape distance (shaders/Chunkmarch.glsl:113), and a point outside the box of the chunk found for it advances tw
//         past that box and stays M_WORLD (:297-330 have no containment check) where the CPU march ends the ray;
//   SEG   the far end: the ray also ends once tw - leaf_back >= far (svo_trace_segments).
#pragma once
#include "march.hip.h"
#include "step_asm.hip.h"

namespace svo {

struct ChunkStepUniform {       // wave-uniform inputs (SGPRs; all of them are held across the march loop for the blocks' sake already)
    V3 wlo, whi;                // the world box
    float csize, eps;
    int cap_chunk, cap_tree;
    const uint32_t *wide;       // (BIG) the wide pool
    decltype(__builtin_amdgcn_kernarg_segment_ptr()) kernarg;   // the launch arguments: TraceArgs::wchunks is read there when the table is not in LDS
};

// The chunk step of every lane in M_WORLD.  All lanes of the wave call this together.  Returns the lanes whose ray ended here (their
// mode is still M_WORLD: the caller stores the record and retires them).  TAB: entries per row of the chunk table in LDS at `lds_tab`.
// G*: the ChunkGrid words as lane values, table_in_lds wave-uniform.
template <bool BIG, bool GLSL, bool SEG>
struct ChunkStepAsm;

#define SVO_CHUNK_WB32 "v_lshlrev_b32 %[wb], 8, %[q6]\n\t"                 // 64 entries of 4 bytes per wide node
#define SVO_CHUNK_WB64 "v_mov_b32 %[q5], 0x100\n\t" "v_mad_u64_u32 %[wb], vcc, %[q6], %[q5], %[widep]\n\t"
#define SVO_CHUNK_CPU_GUARD ""
#define SVO_CHUNK_GLSL_GUARD "v_cmp_gt_f32 vcc, %[eps], %[q1]\n\t" "v_mov_b32 %[q2], 0x3d800000\n\t" "s_nop 0\n\t" "v_cndmask_b32 %[q1], %[q1], %[q2], vcc\n\t"
// miss |= (GLSL ? tw : tw - eps) >= far: EXEC keeps the lanes for which that does not hold (a NaN stays in, as in the C++ block)
#define SVO_CHUNK_FAR_NONE ""
#define SVO_CHUNK_FAR_CPU "v_subrev_f32 %[q1], %[eps], %[tw]\n\t" "v_cmpx_nge_f32 vcc, %[q1], %[far]\n\t"
#define SVO_CHUNK_FAR_GLSL "v_cmpx_nge_f32 vcc, %[tw], %[far]\n\t"

#define SVO_CHUNK_BIG false
#define SVO_CHUNK_WIDE_BASE SVO_CHUNK_WB32
#define SVO_CHUNK_GLSL false
#define SVO_CHUNK_ESCAPE_GUARD SVO_CHUNK_CPU_GUARD
#define SVO_CHUNK_SEG false
#define SVO_CHUNK_FAR_END SVO_CHUNK_FAR_NONE
#include "chunk_step_body.inc"
#undef SVO_CHUNK_SEG
#undef SVO_CHUNK_FAR_END
#define SVO_CHUNK_SEG true
#define SVO_CHUNK_FAR_END SVO_CHUNK_FAR_CPU
#include "chunk_step_body.inc"
#undef SVO_CHUNK_GLSL
#undef SVO_CHUNK_ESCAPE_GUARD
#undef SVO_CHUNK_FAR_END
#define SVO_CHUNK_GLSL true
#define SVO_CHUNK_ESCAPE_GUARD SVO_CHUNK_GLSL_GUARD
#define SVO_CHUNK_FAR_END SVO_CHUNK_FAR_GLSL
#include "chunk_step_body.inc"
#undef SVO_CHUNK_SEG
#undef SVO_CHUNK_FAR_END
#define SVO_CHUNK_SEG false
#define SVO_CHUNK_FAR_END SVO_CHUNK_FAR_NONE
#include "chunk_step_body.inc"
#undef SVO_CHUNK_BIG
#undef SVO_CHUNK_WIDE_BASE
#define SVO_CHUNK_BIG true
#define SVO_CHUNK_WIDE_BASE SVO_CHUNK_WB64
#include "chunk_step_body.inc"
#undef SVO_CHUNK_SEG
#undef SVO_CHUNK_FAR_END
#define SVO_CHUNK_SEG true
#define SVO_CHUNK_FAR_END SVO_CHUNK_FAR_GLSL
#include "chunk_step_body.inc"
#undef SVO_CHUNK_GLSL
#undef SVO_CHUNK_ESCAPE_GUARD
#undef SVO_CHUNK_FAR_END
#define SVO_CHUNK_GLSL false
#define SVO_CHUNK_ESCAPE_GUARD SVO_CHUNK_CPU_GUARD
#define SVO_CHUNK_FAR_END SVO_CHUNK_FAR_CPU
#include "chunk_step_body.inc"
#undef SVO_CHUNK_SEG
#undef SVO_CHUNK_FAR_END
#define SVO_CHUNK_SEG false
#define SVO_CHUNK_FAR_END SVO_CHUNK_FAR_NONE
#include "chunk_step_body.inc"
#undef SVO_CHUNK_BIG
#undef SVO_CHUNK_WIDE_BASE
#undef SVO_CHUNK_GLSL
#undef SVO_CHUNK_ESCAPE_GUARD
#undef SVO_CHUNK_SEG
#undef SVO_CHUNK_FAR_END

} // namespace svo
