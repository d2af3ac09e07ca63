// What crosses the DiffNet translation units on the host side: the plan of a layer-stack launch (which of the six persistent kernels,
// decided ONCE in plan_stack, csrc/diffusion_loop.hip), the launchers that carry it out (csrc/diffnet.hip, csrc/diffnet_x3.hip) and the
// step-boundary launch of the reverse loop (csrc/boundary.hip).
#pragma once
#include "common.h"

// ---- which kernel a stack launch runs ---------------------------------------------------------------------------------
// The values are the ABI's: set_diffnet_stack_variant returns them (include/set_amd.h).
enum StackFamily {
    STACK_DIRECT64 = 0,   // direct fp32 kernel, 64-frame tiles
    STACK_DIRECT32 = 1,   // direct fp32 kernel, 32-frame tiles
    STACK_WINO = 2,       // fp32 Winograd F(2,3) kernel: 64-frame tiles, 8-wave blocks, needs its images and dilation_cycle_length <= 4
    STACK_ROW_SPLIT = 3,  // row-split kernel for small batches: 4 blocks per 32-frame tile, needs its images and the z workspace
    STACK_X3_BF16 = 4,    // split-operand kernel, fp32 = 3 bf16 pieces (six bf16 MFMAs per product; csrc/diffnet_x3.hip)
    STACK_X3_F16 = 5,     // split-operand kernel, fp32 = 2 fp16 pieces (three fp16 MFMAs per product)
};
constexpr int STACK_WINO_MAX_DIL = 8;  // largest dilation of STACK_WINO (WN_MAXD, csrc/diffnet.hip)

struct StackPlan {
    StackFamily family;
    bool split_x2;   // STACK_ROW_SPLIT: the launch on two-piece fp16 operands (diffnet_stack_split_x2_kernel), else the fp32-pipe one
    bool x3_wino;    // STACK_X3_*: Winograd form of GEMM 1 (diffnet_stack_x3v_kernel), else the direct form
    int x3_ncb;      // STACK_X3_*: 32-frame column blocks per tile -- direct 1 or 2, Winograd 2 or 3
    int n_cu;        // CUs of the device the plan was made for
    // the stack reads and writes two-piece fp16 operands: the reverse loop's step boundary then does too
    bool two_piece_fp16() const { return family == STACK_X3_F16 || (family == STACK_ROW_SPLIT && split_x2); }
};

// The plan is made in csrc/diffusion_loop.hip (plan_stack: the ONLY reader of SET_AMD_SPLIT, SET_AMD_SPLIT_F32, SET_AMD_X3, SET_AMD_WINO,
// SET_AMD_STACK_NCB, SET_AMD_X3_TILE and SET_AMD_X3_WINO) and carried out by one of:
int set_launch_diffnet_stack_f32(const SetDiffnetStackArgs &a, const StackPlan &p, hipStream_t s);       // csrc/diffnet.hip: families 0 - 3, fp32 pipe
int set_launch_diffnet_stack_split_x2(const SetDiffnetStackArgs &a, const StackPlan &p, hipStream_t s);  // csrc/diffnet_x3.hip: family 3, split_x2
int set_launch_diffnet_stack_x3(const SetDiffnetStackArgs &a, const StackPlan &p, hipStream_t s);        // csrc/diffnet_x3.hip: families 4, 5

// ---- the reverse loop's step boundary (csrc/boundary.hip) ---------------------------------------------------------------
// may the boundary of this loop run as one launch?  (reads SET_AMD_FUSED_BOUNDARY)
bool boundary_fusable(const SetDiffLoopArgs &a);
// skip sum of Bg utterances -> x_{t-1} in place (eps explicit or Philox at quad_offset) -> next step's stack input (xin_next, NULL after
// the last step); x2: on two-piece fp16 operands; q4 (x2 only): skip and xin_next in the channel-quad layout (common.h, q4f_index)
int launch_boundary(const SetDiffLoopArgs &a, int Bg, const float *skip, float *x, const float *eps, int sid, uint64_t quad_offset,
                    float *xin_next, bool x2, bool q4, hipStream_t s);
// src [Bg][256][T] -> dst in the channel-quad layout: the first step's input projection, once per loop
int launch_relayout_q4(const float *src, float *dst, int Bg, int T, hipStream_t s);
