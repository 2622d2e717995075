// Which kernel runs a 3x3 SAME convolution (host only).  gemm.hip's conv3x3_plan() is the whole decision — every family's coverage rules,
// the tile choice and every selection / tuning knob — and both the launching entry points and the host-only queries
// (ocr_conv3x3_kernel_choice, _accum_supported, _pool_supported, _stats_rows, _bnbwd_rows) read its answer.  The families' files only
// turn a plan into a launch: launch_<family>(plan, operands, stream) picks the template instance the plan names and starts it.
#pragma once
#include "common.h"

enum {   // ConvPlan::family: the codes ocr_conv3x3_kernel_choice reports (k2 / k3 add 1 for tile D, k3 adds 2 for the general-width form)
    CONV_GEMM = 0,       // none of the convolution kernels: the generic GEMM engines (igemm.hip / gemm.hip)
    CONV_HALO = 1,       // conv_halo.hip
    CONV_K2 = 2,         // conv_k2.hip
    CONV_K3 = 4,         // conv_k3.hip
    CONV_WS = 8,         // conv_ws.hip
};
enum {   // epilogue forms beyond the flags (ConvPlan::epi_kind; the kernels' pool_kind)
    CONV_EPI_PLAIN = 0,
    CONV_EPI_POOL12 = 1, // fused 1 x 2 max-pool (feature pairs)
    CONV_EPI_POOL22 = 2, // fused 2 x 2 max-pool
    CONV_EPI_STATS = 3,  // batch-norm statistics of the output: float partials [M / 256][2][Cout]
    CONV_EPI_BNBWD = 4,  // batch-norm backward sums of a masked data gradient: float partials [M / 256][2][Cout]
    CONV_EPI_UNPOOL12 = 5,  // a data gradient routed through the 1 x 2 max-pool in front by its codes: y is [2 M][Cout], nothing at [M]
    CONV_EPI_UNPOOL22 = 6,  // ... through the 2 x 2 max-pool: y is [4 M][Cout]
};

struct ConvPlan {
    int family;                  // CONV_*
    int M, W, H, Cin, Cout;      // the shape it was planned for (M = Nb * W * H pixels)
    int flags, epi_kind;         // EPI_BIAS / _RELU / _MASK / _ACCUM; CONV_EPI_*
    char tile;                   // k2 / k3: 'A' = 256 pixels x 128 channels, 'D' = 256 x 64
    int bn, nw;                  // halo: channels x waves of the workgroup tile (128 / 64 x 4 / 8)
    bool genw;                   // k3: general-width form (tiles cross image boundaries)
    bool single;                 // k3: one 64-channel input chunk (single halo buffer)
    int ws_nc, ws_ksplit;        // ws: image columns per tile, K split inside the workgroup
    int grid, slots, per_slot, xcd_map;   // ws: persistent grid over the pixel tiles
    int prio, stagger, stagger_bit, abl;  // tuning values the kernels take as arguments (halo / k3 MFMA priority; halo stagger; k2 ablation)
    int nst;                     // k2: weight stages
    int choice() const {         // = ocr_conv3x3_kernel_choice
        if (family == CONV_K2) return CONV_K2 + (tile == 'D');
        if (family == CONV_K3) return CONV_K3 + (tile == 'D') + 2 * genw;
        return family;
    }
};
ConvPlan conv3x3_plan(int M, int W, int H, int Cin, int Cout, int flags, int epi_kind);

struct ConvOperands {
    const void* x; const void* wpack; void* y;   // activations [M][Cin], packed weights [Cout][9][Cin], output [M][Cout] (bf16)
    const float* bias; const void* mask;
    void* pool;                                  // CONV_EPI_POOL*: pooled bf16 output; CONV_EPI_STATS / _BNBWD: float partials
    const void* bnz; const float* bn_mean; const float* bn_rstd;   // CONV_EPI_BNBWD: the producer's pre-normalisation output and statistics
    void* codes;                                 // CONV_EPI_POOL* on conv_ws / conv_k3 (ocr_conv3x3_pool_codes_supported): the pool's routing codes
                                                 // uint32 [pooled pixels][Cout / 8]; y may then be NULL (no full-resolution output)
                                                 // CONV_EPI_UNPOOL*: the codes of the pool in front, READ: uint32 [M][Cout / 8]
    int unpool_relu;                             // CONV_EPI_UNPOOL*: the winner's ReLU bit masks the gradient too
};
int launch_halo(const ConvPlan& p, const ConvOperands& o, hipStream_t stream);
int launch_k2(const ConvPlan& p, const ConvOperands& o, hipStream_t stream);
int launch_k3(const ConvPlan& p, const ConvOperands& o, hipStream_t stream);
int launch_ws(const ConvPlan& p, const ConvOperands& o, hipStream_t stream);
