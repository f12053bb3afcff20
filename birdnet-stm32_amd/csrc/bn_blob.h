// bn_blob.h — layout of the packed model blob handed to bn_model_load().
//
// Written by birdnet_stm32/models/_pack.py (which mirrors every constant below) from a
// .keras archive (float32 plan) or a .tflite flatbuffer (INT8 plan).  All integers are
// little-endian; every tensor payload starts on a 256-byte boundary.
//
//   BlobHeader | SlotRec[n_slots] | TensorRec[n_tensors] | OpRec[n_ops] | payloads
//
// A "slot" is an activation buffer; its size is given per chunk and the library allocates
// max_batch times that.  Operators address slots by id; BN_SLOT_INPUT is the caller's input
// tensor, BN_SLOT_SCORES / BN_SLOT_LOGITS the caller's output tensors.
#pragma once
#include <stdint.h>

#define BN_BLOB_MAGIC "BNHIPM01"
#define BN_BLOB_VERSION 5u

#define BN_SLOT_INPUT (-1)
#define BN_SLOT_SCORES (-2)
#define BN_SLOT_LOGITS (-3)
#define BN_SLOT_AUDIO (-4)   // the caller's waveform tensor (operators of the audio path only)
#define BN_SLOT_NONE (-9)

// OpRec.p[BN_OP_PATH]: which entry point runs the operator.  bn_forward starts from the runner-boundary input
// (spectrogram); bn_infer_audio starts from waveforms and may use operators that never materialise the spectrogram.
#define BN_OP_PATH 39
#define BN_PATH_BOTH 0
#define BN_PATH_INPUT 1   // only when starting from BN_SLOT_INPUT
#define BN_PATH_AUDIO 2   // only when starting from BN_SLOT_AUDIO

struct BlobHeader {
    char magic[8];
    uint32_t version;
    uint32_t dtype;        // BN_DTYPE_*
    uint32_t input_kind;   // BN_INPUT_*
    uint32_t input_elems;  // float32 elements per chunk at the runner boundary
    uint32_t fft_bins;
    uint32_t spec_width;
    uint32_t num_classes;
    uint32_t n_slots;
    uint32_t n_tensors;
    uint32_t n_ops;
    uint32_t slots_off;
    uint32_t tensors_off;
    uint32_t ops_off;
    uint32_t reserved;
};
static_assert(sizeof(BlobHeader) == 64, "BlobHeader must be 64 bytes");

struct SlotRec {
    uint64_t bytes_per_chunk;
};

struct TensorRec {
    uint64_t offset;  // from the start of the blob, multiple of 256
    uint64_t nbytes;
};

// OpRec.p[BN_OP_TAIL_TAG]: BN_TAIL_COVERED = the operator is one of the blocks the plan's fused tail operator (BN_OP_I8_TAIL) also
// covers — it is skipped while the tail kernel runs; BN_TAIL_OP marks the tail operator itself, skipped when the option i8_tail is
// off or its maps do not fit the kernel's LDS plan.  Any other value: the operator always runs.
#define BN_OP_TAIL_TAG 38
#define BN_TAIL_COVERED 0x7A110001
#define BN_TAIL_OP 0x7A110002
// BN_FRONT2_HEAD on a BN_OP_F32_FRONT operator: the operator p[BN_OP_FRONT2_DIST] places further on (tagged BN_FRONT2_COVERED) is the
// residual block 32 -> 32 that reads nothing but this operator's output; both may run as one kernel (option f32_front2), which
// writes only the second operator's output.  The packer sets the tags only when no other operator reads the map between them.
#define BN_FRONT2_HEAD 0x7A110003
#define BN_FRONT2_COVERED 0x7A110004
#define BN_OP_FRONT2_DIST 37
// BN_SCALE_HEAD on a BN_OP_I8_SCALE operator: the next operator (tagged BN_SCALE_COVERED) is a plain 1x1 convolution that is the only
// reader of the scaled map; the library may apply the gate while that convolution loads its input (i8_pw_wave_kernel) and skip the MUL.
#define BN_SCALE_HEAD 0x7A110005
#define BN_SCALE_COVERED 0x7A110006
// BN_SEGATE_HEAD on a BN_OP_I8_MEAN operator: the next two operators (tagged BN_SEGATE_COVERED) are the FULLY_CONNECTED layers of a
// squeeze-excite gate, each the only reader of its predecessor: pooling and both layers may run as one kernel per chunk.
#define BN_SEGATE_HEAD 0x7A110007
#define BN_SEGATE_COVERED 0x7A110008
// BN_PWDW_HEAD on a plain 1x1 BN_OP_F32_DWPW operator (the expand convolution of an inverted-residual block): the next operator
// (BN_OP_F32_DW, tagged BN_PWDW_COVERED) is the only reader of its output and may run inside the same kernel (f32_pwdw_kernel)
#define BN_PWDW_HEAD 0x7A110009
#define BN_PWDW_COVERED 0x7A11000A
// BN_PWDW_STEM on a BN_OP_F32_STEM operator: the next two operators are a BN_PWDW_HEAD / BN_PWDW_COVERED pair that is the only reader of the
// stem map; the fused kernel may compute the stem rows itself (the stem map is never written)
#define BN_PWDW_STEM 0x7A11000B
// the INT8 counterpart: BN_PWDW8_HEAD on a plain 1x1 BN_OP_I8_DWPW operator, BN_PWDW8_COVERED on the BN_OP_I8_DW operator behind it (i8_pwdw_kernel)
#define BN_PWDW8_HEAD 0x7A11000C
#define BN_PWDW8_COVERED 0x7A11000D
// BN_MID_COVERED / BN_MID_OP: the same pair of tags as BN_TAIL_COVERED / BN_TAIL_OP for the fused stage-2 chain (BN_OP_I8_MID, option i8_mid)
#define BN_MID_COVERED 0x7A11000E
#define BN_MID_OP 0x7A11000F

// OpRec.p[BN_OP_EMB_TAG] = BN_EMB_OP: the operator's result is the model's embedding, the pooled vector that feeds the classifier head
// (INT8 MEAN / attention pooling, float32 GAP / attention pooling) — or, on a fused operator (BN_OP_I8_TAIL, BN_OP_F32_GAPDENSE), the
// vector it pools on chip.  p[BN_OP_EMB_DIM] = its width D; INT8 plans: p[BN_OP_EMB_ZP] = its zero point, f[BN_OP_EMB_SCALE] = its scale.
// Only the kinds above carry the tag, so the three p slots and the f slot are free on them.  Squeeze-excite MEANs are never tagged.
#define BN_OP_EMB_TAG 36
#define BN_OP_EMB_DIM 35
#define BN_OP_EMB_ZP 34
#define BN_OP_EMB_SCALE 7
#define BN_EMB_OP 0x7A110010

#define BN_OP_NP 40
#define BN_OP_NT 16
#define BN_OP_NF 8

struct OpRec {
    int32_t kind;
    int32_t in0;   // slot id
    int32_t in1;   // slot id (residual / gate) or BN_SLOT_NONE
    int32_t out;   // slot id
    int32_t p[BN_OP_NP];
    int32_t t[BN_OP_NT];  // tensor ids, -1 = absent
    float f[BN_OP_NF];
};
static_assert(sizeof(OpRec) == 16 + 4 * BN_OP_NP + 4 * BN_OP_NT + 4 * BN_OP_NF, "OpRec packing");

// ---------------------------------------------------------------------------------------
// Operator kinds.  Activations are NHWC per chunk (C innermost); P = H*W positions.
// What p[], t[] and f[] hold for each kind — names, order, shapes and meaning — is defined in bn_ops.h (namespace bn::op::<kind>)
// and nowhere else; the entries above (BN_OP_PATH, BN_OP_TAIL_TAG, BN_OP_FRONT2_DIST, BN_OP_EMB_*) are the same for every kind.
// ---------------------------------------------------------------------------------------
enum BnOpKind : int32_t {
    // ---- float32 plan --------------------------------------------------------------
    BN_OP_F32_MEL = 1,        // spectrogram -> mel map (band-sparse mixer)
    BN_OP_F32_MAG = 2,        // in place: max normalisation + magnitude scaling
    BN_OP_F32_RAWFE = 3,      // waveform -> raw-frontend map
    BN_OP_F32_STEM = 4,       // 3x3 stem convolution (one input channel)
    BN_OP_F32_DW = 5,         // depthwise 3x3
    BN_OP_F32_PW = 6,         // pointwise 1x1 (+ residual, + squeeze-excite gate)
    BN_OP_F32_SEGATE = 7,     // squeeze-excite gate: pool + two dense layers
    BN_OP_F32_SCALE = 8,      // map * gate
    BN_OP_F32_GAP = 9,        // global average pool
    BN_OP_F32_DENSE = 10,     // classifier head
    BN_OP_F32_ATTNPOOL = 11,  // attention pooling
    BN_OP_F32_DWPW = 12,      // fused [depthwise 3x3 ->] pointwise 1x1 on the matrix cores
    BN_OP_F32_STFTMEL = 13,   // audio -> un-normalised mel energies (STFT with the mixer fused)
    BN_OP_F32_MELFIN = 14,    // un-normalised mel energies -> frontend output
    BN_OP_F32_FRONT = 15,     // stem -> depthwise stride 2 -> pointwise, one kernel
    BN_OP_F32_GAPDENSE = 16,  // global average pool + classifier head, one kernel

    // ---- INT8 plan -----------------------------------------------------------------
    BN_OP_I8_QUANT = 20,     // float32 spectrogram -> int8
    BN_OP_I8_MEL = 21,       // mel mixer (generic kernel)
    BN_OP_I8_STEM = 22,      // 3x3 stem convolution
    BN_OP_I8_DW = 23,        // depthwise 3x3
    BN_OP_I8_PW = 24,        // pointwise 1x1 (+ residual ADD)
    BN_OP_I8_MEAN = 25,      // MEAN over the positions
    BN_OP_I8_FC = 26,        // FULLY_CONNECTED (+ LOGISTIC table)
    BN_OP_I8_HEAD = 27,      // int8 classifier output -> float32 scores (+ logits)
    BN_OP_I8_DWPW = 28,      // fused [depthwise 3x3 ->] pointwise 1x1 on the int8 matrix cores; also the mel mixer
    BN_OP_I8_FRONT = 29,     // stem -> depthwise stride 2 -> pointwise, one kernel
    BN_OP_I8_TAIL = 30,      // the back half of the graph in one kernel (bn_i8_tail.hip, bn_i8_tail2.hip)
    BN_OP_I8_SCALE = 31,     // squeeze-excite MUL: map * gate
    BN_OP_I8_MAXNORM = 32,   // per-chunk max normalisation (+ per-channel table)
    BN_OP_I8_RAWFE = 33,     // raw frontend of an exported graph
    BN_OP_I8_ATTNPOOL = 34,  // attention pooling of an exported graph
    BN_OP_I8_MID = 35,       // the three blocks of stage 2 in one kernel (bn_i8_tail2.hip: i8_mid2_kernel)
};
