/*
 * graphinvent_amd.h — C ABI of libgraphinvent_amd.so (gfx950 / MI355X only).
 *
 * Drop-in boundary.  The reference has NO native layer: its GGNN hot path
 * (graphinvent/gnn/summation_mpnn.py:80-149, gnn/mpnn.py:229-303, gnn/modules.py:12-52,111-281) is
 * stock PyTorch called as `model(nodes, edges)` from Workflow.py:785,826, GraphGenerator.py:121,
 * GraphGeneratorRL.py:131-132 and Analyzer.py:759.  The Python boundary therefore stays the
 * reference's own — `gnn.mpnn.GGNN(constants).forward(nodes, edges)` — and this header is what
 * that class binds underneath (ctypes, graphinvent_amd/lib.py).  Each entry point names the
 * reference statement(s) it replaces.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller (torch tensors passed by data_ptr());
 *     nothing here allocates or frees; workspaces are caller provided;
 *   - matrices are fp32 row-major with an explicit leading dimension in floats; index arrays
 *     are int32;
 *   - `stream` is a hipStream_t; all work is enqueued asynchronously on it;
 *   - return value: 0 = success, >0 = hipError_t from a launch, <0 = argument error (GI_E*);
 *   - no exceptions cross the ABI; one process per GPU, calls come from one host thread at a time.
 *     Process-wide state is limited to: the optional per-launch timing log (gi_prof_*), a pool of
 *     timing-disabled hipEvents used to order the backward's two streams, the test / measurement hooks
 *     gi_gemm_config and gi_mlp_chain_config, and eight switches read from the environment:
 *       GI_BF3=0                every GEMM and chain on the fp32 MFMA (default 1: the node-level readout layers >= 192
 *                               wide and the message stacks' chains, forward and dZ, run as splits on the 16-bit MFMA
 *                               pipe, GI_GEMM_BF3 — same result to ~3e-7; gi_bf3_enable)
 *       GI_X2=0                 those launches as three bf16 planes (six products) instead of two scaled fp16 planes
 *                               (three products, GI_GEMM_X2; gi_x2_enable); also puts the chains back on fp32
 *       GI_FUSE=<mask>          launch-count reductions (gi_fuse_flags, default 15)
 *       GI_GLUE=<mask>          small launches folded into their neighbours (gi_glue_flags, default GI_GLUE_DEFAULT)
 *       GI_B3P=0, GI_B3V=0      initial values of gi_b3p_enable / gi_b3v_enable (default 1)
 *       GI_B3P_ALL=1            forward / dgrad launches on the software-pipelined kernel whatever their tile count
 *                               (default: from 2.5 tiles per CU on; gi_b3p_enable)
 *       GI_CHAIN_PACK_FUSED=0   the fp16x2 chain image as memset + gi_absmax + pack launches instead of one launch that
 *                               also writes the max |W| cells (read per call: the test of the fused launch compares both)
 *       GI_X2N=0                fp16x2 forward / dgrad launches on gi_gemm_bf3_kernel instead of the column-split kernel
 *                               (the same results bit for bit; read per launch: its test compares both)
 *       GI_GEMM_LOG=<file>      one line per GEMM launch (tools/gemm_launch_report.py); output only
 *     Variants that were measured and not adopted are in the git history, not behind switches
 *     (tools/experiments/README.md, "Retired switches").
 */
#ifndef GRAPHINVENT_AMD_H
#define GRAPHINVENT_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define GI_ABI_VERSION 18
#define GI_MAX_GROUPS 8       /* max bond types (n_edge_features) */
#define GI_MAX_NODES 128      /* max max_n_nodes */
#define GI_P0_MAX_CLASSES 256 /* max distinct node feature rows for the pass-0 shortcut */

#define GI_DTYPE_F32 0        /* element type of model INPUTS (nodes, edges, APD targets): fp32 ... */
#define GI_DTYPE_I8  1        /* ... or the int8 the preprocessed HDF stores (DataProcesser.py:157-161) */

#define GI_EINVAL   (-1)      /* bad dims / null pointer */
#define GI_ELIMIT   (-2)      /* exceeds a compiled-in limit */

int gi_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * K1 graph_compact — replaces the dense->sparse bookkeeping of gnn/summation_mpnn.py:100-124
 * (`edges.sum(3)`, two `nonzero`s, the [V,E] 0/1 summation matrix, `edges[eb,ei,ej,:]`, the
 * zero-padded `hidden_nodes`) and `node_mask` (:146).
 *
 * MESSAGE ROWS.  The message an edge carries, MLP_type(e)(h_src(e)) (gnn/mpnn.py:284-294), depends
 * only on (source node, bond type); it is computed once per distinct pair: U <= E rows (0.55-0.63 E
 * on molecular graphs), bond-type-major, inside a type by source slot.
 *
 * Layout of the fixed-size int32 index buffer `gfix` (offsets in ints, from gi_compact_layout):
 *   counts[GI_COUNTS]  [0]=S active node slots, [1]=E directed edges, [2]=error flag (an edge whose
 *                feature vector is not one-hot), [3]=U message rows, [4+t]=message rows of bond
 *                type t, [12+t]=edges of bond type t, [20]=D0 pass-0 rows (0 = shortcut off)
 *   type_off[GI_MAX_GROUPS+1] (message rows per bond type, prefix), cidx[B*N] (slot -> compact row,
 *   S for inactive slots), node_mask[B*N] (1 if the slot has >=1 incoming edge), slot_of[B*N],
 *   seg_off[B*N+2] (dst-CSR over compact rows: row c's incoming edges are slots
 *   [seg_off[c], seg_off[c+1]); row S empty), src_off[B*N+2] (source CSR over MESSAGE rows: row c
 *   sends out_perm[src_off[c] .. src_off[c+1])), then scratch.
 * Variable-size arrays (caller-allocated once S, E, U are known, written by gi_compact_fill):
 *   u_src[U]    message row -> source compact row (the message MLP's gather index)
 *   in_perm[E]  dst-CSR slot -> message row (edges in the reference's order: row-major nonzero)
 *   mu_off[U+1], mu_dst[E], mu_slot[E]   message row -> its edges: destination compact row and
 *               dst-CSR slot of each, ascending destination (backward of the aggregation)
 *   out_perm[U] message rows grouped by source compact row, inside a row by bond type
 * PASS-0 ROWS.  At the first message pass h = [x | 0..0], so a message row depends only on (feature
 * row of its source, bond type): D0 rows (atom type x charge x bond type; counts[20]), bond-type-
 * major with offsets type_off0[GI_MAX_GROUPS+1] in gfix.  d_src[D0] = a compact row of each class
 * (the MLP's gather index); cmat[S+1, ldc0] fp32 = number of edges into each compact row from each
 * pass-0 row, so that the pass-0 aggregation is cmat . m0 and its backward cmat^T . d agg.
 * ------------------------------------------------------------------------------------------ */
#define GI_COUNTS 24
#define GI_DIMS 8             /* device-side launch dimensions of a bounded forward (gi_compact_bound) */
typedef struct gi_compact_layout_t {
    int total_ints;
    int counts, type_off, cidx, node_mask, slot_of, seg_off, src_off, type_off0, scratch;
    int dims;
} gi_compact_layout_t;

int gi_compact_layout(int B, int N, int Fe, gi_compact_layout_t* out);

/* phase 1: per-graph counting + global scans; fills everything in gfix. */
int gi_compact_count(const void* nodes, const void* edges, int in_dtype, int B, int N, int Fn,
                     int Fe, int* gfix, void* stream);
/* nodedup != 0: NO row sharing — every slot of the [B, N] grid is a compact row of its own (S = B*N;
 * padded slots too), every edge its own message row (U = E, ordered bond type, source slot,
 * destination), no pass-0 rows (D0 = 0).  The layout AlphaDropout's training mode needs (an
 * independent mask per edge and per padded slot, gnn/modules.py:130-142); counts[23] records the
 * mode for gi_compact_fill.  nodedup == 0 is gi_compact_count. */
int gi_compact_count_ex(const void* nodes, const void* edges, int in_dtype, int B, int N, int Fn,
                        int Fe, int* gfix, int nodedup, void* stream);
/* BOUNDED (host-sync-free) forward, between phase 1 and phase 2: instead of reading S, E, U, D0 back the
 * caller sizes every buffer for bounds (S <= B*N; E, U <= e_bound; D0 <= d0_bound) and this one-thread launch
 * checks the counted sizes against them and derives the launch dimensions the forward's kernels read on the
 * device: gfix[layout.dims + 0] = R = S + 1, + 1 = row-block height of the message chains, + 2 = 32.  On a
 * violation — more edges / pass-0 rows than the bound (counts[2] |= 2), or a batch with edges whose pass-0
 * shortcut is unavailable (node features not 0/1, counts[2] |= 4) — every size is set to 0: the forward then
 * stays inside its buffers and returns meaningless logits; read counts[2] at the next synchronisation.
 * `sticky_err` (may be NULL): a caller-owned device int that accumulates (atomic OR) the error bits of every
 * bounded forward — counts[2] lives in that forward's own gfix, so a loop that checks once at its end would
 * otherwise see only the last round (bit 0 = an edge's feature vector is not one-hot, from phase 1).
 * This is what a caller that mutates `nodes` / `edges` in place between forwards
 * (GraphGenerator.build_graphs, GraphGenerator.py:118-157) needs: no device -> host wait per forward. */
int gi_compact_bound(int* gfix, int B, int N, int Fe, int e_bound, int d0_bound, int* sticky_err, void* stream);
/* phase 2 (after the host has read S, E, U from counts): the variable-size index arrays and the
 * initial node rows hx0[S+1, ldhx] = [x | 0.. | x] with the input features in columns [0,Fn) and
 * again in [H, H+Fn) (row S = 0).  S < 0: bounded mode — E, U, D0 (and the buffers) are the bounds handed to
 * gi_compact_bound, the real sizes are read from gfix on the device. */
int gi_compact_fill(const void* nodes, int in_dtype, int B, int N, int Fn, int Fe, const int* gfix,
                    int S, int E, int U, int* u_src, int* in_perm, int* mu_off, int* mu_dst,
                    int* mu_slot, int* out_perm, float* hx0, int ldhx, int H, int D0, int* d_src,
                    float* cmat, int ldc0, int* e2d, void* stream);
/* AttentionGGNN's pass 0 on the D0 class rows: e2d[E] (written by gi_compact_fill when non-NULL and
 * D0 > 0) = dst-CSR edge slot -> pass-0 row, the index the segment softmax reads its rows through;
 * gi_compact_class_csr turns it into the CSR pass-0 row -> its edge slots (cls_off[D0+1],
 * cls_edges[E], slots ascending: fixed summation order) over which the softmax backward is summed. */
int gi_compact_class_csr(const int* e2d, int E, int D0, int* cls_off, int* cls_edges, void* stream);

/* The compacted graph as the fused model calls take it. */
typedef struct gi_graph {
    int S, E, U;
    const int* gfix;
    const int* u_src; const int* in_perm; const int* mu_off; const int* mu_dst; const int* mu_slot;
    const int* out_perm;
    const int* Ut;            /* HOST array [Fe]: message rows per bond type (counts[4..4+Fe)) */
    int D0, ldc0;             /* pass-0 rows (0 = shortcut off) and leading dimension of cmat */
    const int* d_src;         /* [D0] */
    const float* cmat;        /* [S+1, ldc0] */
    const int* e2d;           /* [E]    AttentionGGNN pass 0 (NULL: that pass runs on message rows) */
    const int* cls_off;       /* [D0+1] */
    const int* cls_edges;     /* [E] */
    int bounded;              /* != 0: host-sync-free forward — S, E, U, D0, Ut[] above are upper BOUNDS (the
                                 sizes every buffer was allocated for); the real sizes stay on the device in
                                 gfix (gi_compact_bound) and every kernel of gi_ggnn_forward reads them there.
                                 Forward only (gi_ggnn_backward needs host sizes), no dropout mode. */
    void* p0_cache;           /* NULL, or gi_p0_cache_words() 4-byte words of device memory (16-byte aligned,
                                 zero-filled = empty) that OUTLIVE the call: the pass-0 row cache of an
                                 inference loop, see gi_p0_cache_words.  Forward only (the hidden activations
                                 of the pass-0 stacks are not produced on a hit). */
    int* x2_guard;            /* NULL, or GI_X2_GUARD_WORDS device ints that OUTLIVE the call: sticky counters of the
                                 fp16x2 dynamic-range guard (see GI_GEMM_X2 / gi_gemm_params.x2_guard):
                                 [0] rows of a FORWARD launch's activation operand whose largest magnitude lies more
                                     than 2^24 below the tensor's (such a row keeps fewer than ~14 bits in fp16x2),
                                 [1] rows / columns of a weight matrix of those layers in the same position,
                                 [2] the same for the dZ operands of the dgrad launches (informational: everything the
                                     backward outputs is a sum over rows, which an absolute error floor of 2^-38 of the
                                     tensor's maximum does not move),
                                 [3] reserved (stays 0). */
    int* x2_guard_host;       /* NULL, or ONE int of host memory mapped into the device (gi_host_flag_create): set to 1
                                 by the launch that increments counter [0] or [1], so that the host learns of a trip
                                 without a read-back and can run the following calls with GI_RUN_NO_X2 */
    float* wcache;            /* NULL, or gi_ggnn_wcache_floats() floats of device memory (16-byte aligned) that OUTLIVE the
                                 call: everything a FORWARD derives from the weights alone — the fp16x2 forward chains'
                                 two-plane weight image and their max |W| cells, max |W| of the node-level fp16x2 layers —
                                 kept across forwards of an inference / generation loop (round 6).  Forward only
                                 (gi_ggnn_backward does not read it: pass a graph without it to a forward that needs a tape). */
    int wcache_valid;         /* with wcache: 0 = (re)derive everything into it now (first forward, or the weights /
                                 the arithmetic switches changed since: the CALLER keeps that key), != 0 = its contents
                                 match the weights: no pack, no amax pass, no weight guard launches */
} gi_graph;
#define GI_X2_GUARD_WORDS 4
/* One int of pinned host memory that kernels can write (hipHostMalloc mapped): *host = the caller's view,
 * *dev = the pointer to hand to kernels (gi_graph.x2_guard_host).  Zeroed on creation. */
int gi_host_flag_create(int** host, int** dev);
int gi_host_flag_destroy(int* host);

/* ------------------------------------------------------------------------------------------
 * Dense GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32) with fused prologue/epilogue.  One kernel
 * family serves
 *   forward  Y = selu(X[a_idx] W^T + b)      torch.nn.Linear + SELU, gnn/modules.py:130-142,166-170
 *   dgrad    dX = (dZ W) * selu'(Xact)        autograd of the same
 *   wgrad    [dW | db] = dZ^T [X[b_idx] | 1]  autograd of the same (split over rows, slabs)
 * grouped per bond type (gnn/mpnn.py:284-294 evaluates all Fe MLPs on all edges and masks; here
 * every edge row only meets its own type's weights).
 * ------------------------------------------------------------------------------------------ */
#define GI_EPI_BIAS    1   /* v += bias[col]                                 */
#define GI_EPI_SELU    2   /* v = selu(v)                                    */
#define GI_EPI_DSELU   4   /* v *= selu'(act[row,col]) (act = selu output)   */
#define GI_EPI_ACCUM   8   /* v += C[row,col]                                */
#define GI_GEMM_SPLITK 16  /* reduction range partitioned by groups/splits; C is a slab set */
#define GI_EPI_MULACT  64  /* v *= act[row,col] (a stored factor: AlphaDropout training mode) */
#define GI_GEMM_BF3    128 /* B is a pre-split bf16 image (gi_bf3_pack); the launch runs on the bf16 MFMA pipe with
                              fp32 operands split three ways (six bf16 products per fp32 product, fp32 accumulate:
                              the same result to ~4e-7 relative, the fp32 MFMA chain's own distance from the fp64 product).  A contig fp32, no groups / split-K / a_idx / b_idx
                              (32-bit operand offsets: a gathered row is not bounded by M), K < 4 needs lda / ldb >= 4;
                              every problem of a batched launch or none */
#define GI_GEMM_BF3B_F32 512 /* with GI_GEMM_BF3: B is the plain fp32 matrix [N][ldb] (a forward weight as stored), split while
                              it is staged like A: no image, 4 bytes per element through L2 instead of 6 */
#define GI_GEMM_BF3A   256 /* with GI_GEMM_BF3: A is a pre-split bf16 image too ([3][M][Kp], gi_bf3_pack of an [M, K]
                              matrix or the `planes` output of a producing launch); no a_idx */
#define GI_GEMM_T128  2048 /* with GI_GEMM_BF3 | GI_GEMM_X2, weight-gradient layout: prefer the 128 x 128-tile kernel (256 threads,
                              32 KB of LDS, several workgroups per CU: gi_gemm_b3v.hip) to the software-pipelined
                              128 x 256-tile one (one 512-thread workgroup per CU) — launches of many small problems.
                              Callers' choice: gi_ggnn_backward never sets it */
#define GI_GEMM_X2    1024 /* with GI_GEMM_BF3 and plain fp32 operands: split every operand into TWO scaled fp16 values
                              instead of three bf16 (csrc/gi_x2.h): three f16 MFMA products per fp32 product instead of
                              six, the same ~3e-7 distance from the fp64 product.  Needs the largest magnitude of both
                              operand tensors on the device (`a_amax`, `b_amax`: written by the `c_amax` of the launch
                              that produced the tensor, or by gi_absmax) */

typedef struct gi_gemm_params {
    const float* A; const float* B; float* C;
    const float* bias; const float* act;
    const int* a_idx; const int* b_idx;   /* gather on the STORED rows of A / B, or NULL */
    const int* grp_off;                   /* device [ngroups+1] or NULL */
    int M, N, K;                          /* output M x N, reduction length K */
    int lda, ldb, ldc, ldact;
    int flags;                            /* GI_EPI_* | GI_GEMM_SPLITK | GI_GEMM_BF3 */
    int a_major, b_major;                 /* operand stored [reduction][rows] instead of [rows][reduction] */
    int tm, tn;                           /* block tile = 64*tm x 64*tn, (tm,tn) in {(1,1),(1,2),(2,2)} */
    int ngroups, nsplit;                  /* ngroups 0 = ungrouped; nsplit >= 1 */
    int max_group_rows;                   /* host upper bound of rows per group (grid sizing) */
    int ones_col;                         /* B stored column that reads as 1.0 (bias-grad column), -1 = none */
    long long c_split_stride;             /* floats between split slabs */
    const float* Bg[GI_MAX_GROUPS]; const float* biasg[GI_MAX_GROUPS]; float* Cg[GI_MAX_GROUPS];
    int gsplit[GI_MAX_GROUPS];            /* grouped split-K: slabs of group g (>= 1 each); nsplit ignored */
    /* Bounded (host-sync-free) launches: M (and K) are then UPPER BOUNDS that size the grid, the real
     * extents are read on the device — rows = min(M, *m_dev), reduction length = min(K, *k_dev); output
     * tiles beyond the real rows exit at once.  NULL: M / K as given.  Not with groups or split-K. */
    const int* m_dev; const int* k_dev;
    /* GI_GEMM_X2: the "amax cells" (GI_AMAX_WORDS floats each, see below) holding max |A|, max |B|, read when the kernel
     * starts.  c_amax (any launch, may be NULL): the cell that receives max |C| over everything this launch stores —
     * the caller zeroes the cell before the producer runs. */
    const float* a_amax; const float* b_amax;
    float* c_amax;
    /* GI_GEMM_X2 launches with a row-major A (forward / dgrad layouts), optional: dynamic-range guard.  The launch counts
     * in x2_guard[0] the rows of A whose largest magnitude is non-zero and more than 2^24 below max |A| (a row the
     * per-TENSOR scale leaves with fewer than ~14 significant bits; an exactly-zero row is exact; every row is counted
     * once per launch) and, when it counted a row and x2_guard_host != NULL, stores 1 there. */
    int* x2_guard; int* x2_guard_host;
} gi_gemm_params;

int gi_gemm(const gi_gemm_params* p, void* stream);
/* An amax cell: GI_AMAX_WORDS floats, the tensor's largest magnitude = the maximum over the cell (writers spread their
 * atomic max over 64 slots one 128-byte line apart, csrc/gi_x2.h; all values >= 0, a zeroed cell = "nothing yet"). */
#define GI_AMAX_WORDS 2048
/* max |x| of up to GI_ABSMAX_MAX matrices [rows][cols] (pitch ld) in one launch, maxed into the amax cell `out` (zero it
 * first) — the weights' side of GI_GEMM_X2 (their other operands get theirs from the producing launch's c_amax). */
#define GI_ABSMAX_MAX 16
typedef struct { const float* x; int rows, cols, ld; float* out; } gi_absmax_desc;
int gi_absmax(const gi_absmax_desc* descs, int n, void* stream);
/* fp16x2 dynamic-range guard of weight matrices (descs[i].out = the matrix's amax cell, already filled by gi_absmax on
 * this stream): counts in *counter the ROWS and COLUMNS whose largest magnitude is non-zero and more than 2^24 below
 * the matrix's — an output channel of the forward (row of W) or of the dgrad (column of W) launch that the per-tensor
 * scale leaves with fewer than ~14 significant bits — and stores 1 to *host_flag (may be NULL) when it counted one. */
int gi_x2_weight_guard(const gi_absmax_desc* descs, int n, int* counter, int* host_flag, void* stream);
/* n (<= 8) independent problems of the same tile shape and operand layouts in ONE launch.
 * Every launch is a tile loop: launches with more output tiles than the device holds workgroups at once
 * run as a persistent grid (each workgroup walks tiles id, id + grid, ...; the next tile's first operand
 * loads are issued in front of the current tile's epilogue).  Operands are addressed with 32-bit byte
 * offsets from their base pointers: every matrix must span less than 4 GB (GI_ELIMIT otherwise). */
int gi_gemm_batch(const gi_gemm_params* problems, int n, void* stream);
/* Measurement / test hook (process-wide): persist_tenths >= 0 sets the persistent-grid threshold in tenths of
 * a full round of resident workgroups (default 0 = one workgroup per tile: the persistent grid measured a tie alone
 * and a loss beside the weight-gradient stream);
 * grid_cap > 0 caps every launch at that many workgroups (0 = no cap). */
int gi_gemm_config(int persist_tenths, int grid_cap);   /* returns 0 */

/* ------------------------------------------------------------------------------------------
 * Resident-activation MLP chain — a whole `MLP.forward` (gnn/modules.py:166-170: Linear -> SELU for
 * every layer including the last) of the per-bond-type message / attention stacks
 * (`GGNN.message_terms` gnn/mpnn.py:284-294, `AttentionGGNN.aggregate_message` gnn/mpnn.py:370-389),
 * or the whole dZ chain of its backward, in ONE launch: each workgroup carries 32 rows through all
 * layers with the activation tile resident in LDS; every layer's output is also written to `out`.
 *   forward : layer l: out_l[rows, N] = selu(in_l W_l^T + bias_l),   W_l = [N][K] row-major
 *   backward: layer l: out_l[rows, N] = (in_l W_l) * selu'(act_l),   W_l = [K][N] row-major
 *             (act_l NULL: no SELU factor — the input gradient of the stack's first Linear)
 * in_0 = X rows (optionally gathered by x_idx), in_{l+1} = out_l.  Rows are grouped like gi_gemm's
 * grouped problems (group t uses W[t] / bias[t]; `grp_off` on the device, `group_rows` = host upper
 * bounds for the grid).  Limits: nlayers <= GI_CHAIN_MAXL, 4 <= K, N <= GI_CHAIN_MAXW (GI_ELIMIT
 * otherwise — callers then run the stack layer by layer through gi_gemm).
 * ------------------------------------------------------------------------------------------ */
#define GI_CHAIN_MAXL 8
#define GI_CHAIN_MAXW 256
typedef struct {
    const float* W[GI_MAX_GROUPS];
    const float* bias[GI_MAX_GROUPS];     /* forward only */
    float* out; int ldo;
    const float* act; int ldact;          /* backward only */
    int K, N;
    float* out_amax;                      /* NULL, or an amax cell (GI_AMAX_WORDS floats, csrc/gi_x2.h): the fp16x2 chain kernels
                                             (x2_wamax != NULL) publish max |out| of this layer over ALL groups into it — what
                                             the fp16x2 weight-gradient launches of the stack scale their operands with
                                             (activations: forward chain, dZ: backward chain).  Ignored by the fp32 chain. */
} gi_chain_layer;

typedef struct {
    gi_chain_layer layer[GI_CHAIN_MAXL];
    int nlayers;
    const float* X; int ldx;              /* ldx >= round-up-to-4(layer[0].K) */
    const int* x_idx;                     /* row gather for X, or NULL */
    const int* grp_off;                   /* device: ngroups + 1 row offsets (NULL: one group, rows [0, rows)) */
    int ngroups;
    int group_rows[GI_MAX_GROUPS];        /* host upper bound of rows per group */
    int rows;                             /* total rows */
    int backward;
    float* image;                         /* packed weight image, gi_mlp_chain_image_floats() floats,
                                             16-byte aligned; filled by gi_mlp_chain_pack */
    long long image_stride;               /* floats per group in the image; 0 = that of THESE layers.
                                             A chain that runs only the first layers of a packed
                                             stack passes the stride of the full pack. */
    const int* skip_flag;                 /* NULL, or a device int read at kernel start: != 0 -> the launch does
                                             nothing (gi_ggnn_forward: pass-0 rows served from gi_graph.p0_cache) */
    const int* tile_rows_dev;             /* bounded (host-sync-free) launch, else NULL: device int holding the
                                             row-block height (32..36).  `rows` is then an upper BOUND of the
                                             rows of all groups together (sizes the grid), the real row ranges
                                             come from grp_off on the device (required), group_rows is unused */
    float* x2_wamax;                      /* NULL, or nlayers x ngroups amax cells (GI_AMAX_WORDS floats each, [layer][group]):
                                             the fp16x2 chain (csrc/gi_x2.h) — gi_mlp_chain_pack computes max |W| of
                                             every layer and group into them and writes the image as two scaled fp16
                                             planes; gi_mlp_chain then runs 64-row blocks on the f16 MFMA pipe (three
                                             products per fp32 product, activations scaled per 64-ROW BLOCK and layer by
                                             a power of two from the block's largest magnitude: a row's last bits
                                             depend on which rows share its block — NOT bitwise row-independent like
                                             the fp32 chain: gi_ggnn_backward's dZ chains run this way, gi_ggnn_forward
                                             uses x2_rows32 below).  Pack and launch must agree; a
                                             bounded launch walks 64-row blocks (the value behind tile_rows_dev is unused) */
    float* x_amax;                        /* NULL, or an amax cell for max |X rows read| (after the x_idx gather; all groups) —
                                             published by the fp16x2 chain kernels like layer[].out_amax */
    int x2_rows32;                        /* with x2_wamax: != 0 = the ROW-INDEPENDENT fp16x2 chain — 32-row blocks, every row
                                             of the activation tile scaled by its OWN power of two (the product is formed
                                             transposed, so that a lane holds one row: its maximum is an in-register
                                             reduction), outputs staged through LDS and stored as whole rows.  A row's
                                             result depends on the row and the weights only, bit for bit, like the fp32
                                             chain's: what gi_ggnn_forward uses for the message rows.  Same packed image as
                                             the 64-row variant.  Launches of more row blocks than the chip has CUs run
                                             two workgroups per CU (a build of the kernel with half the LDS). */
} gi_chain_params;

/* The kernel streams the weights as a pre-packed image (one linear stream of 32 KB LDS tile images per
 * group, zero padded, all layers back to back): gi_mlp_chain_pack writes it from layer[].W (needs
 * nlayers, ngroups, backward, K/N/W of every layer and `image`); it stays valid until the weights
 * change, for any rows / X / out of the same stack. */
/* ------------------------------------------------------------------------------------------
 * Operand image for GI_GEMM_BF3 launches: the three bf16 planes [rows][Kp] (Kp = cols rounded up to 32, zero
 * padded) of a weight matrix, one plane after the other — B[n][k] = W[n * ld + k], or W[k * ld + n] with
 * `transpose` (dgrad of a torch.nn.Linear weight [out, in]: rows = in, cols = out, ld = in).  Valid until the
 * weights change.  `image`: gi_bf3_image_elems(rows, cols) 2-byte elements, 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
#define GI_BF3_PACK_MAX 16
#define GI_BF3_DEFAULT 1    /* gi_ggnn_forward / backward: node-level readout layers >= 192 wide on GI_GEMM_BF3 launches
                              (environment GI_BF3=0 / 1 overrides) */
typedef struct {
    const float* W; int rows, cols, ld; int transpose;
    unsigned short* image;
    int as_f32;               /* != 0: write B as plain fp32 [rows][(cols + 3) & ~3] instead of the three planes (for
                                 GI_GEMM_BF3B_F32 launches: a transposed copy of a weight, 4 bytes per element through L2
                                 instead of 6); fits the same buffer */
} gi_bf3_pack_desc;
/* Which kernel runs a GI_GEMM_BF3 launch whose operands are plain fp32 (test hooks; on = 1 / 0 sets, on < 0
 * queries; both return the previous setting; environment GI_B3P / GI_B3V set the initial values, default 1):
 *   gi_b3p_enable: the software-pipelined 128 x 256 kernel (gi_gemm_b3p.hip) — weight-gradient launches
 *                  (a_major + b_major + split-K slabs; autograd of gnn/modules.py:166-170) always, forward / dgrad
 *                  launches from 2.5 tiles per CU on;
 *   gi_b3v_enable: the 32-deep-tile 128 x 128 kernel (gi_gemm_b3v.hip) for what is left (dgrad with W as stored);
 * everything else — and everything when both are off — runs on the round-3 kernel (gi_gemm_bf3.hip). */
int gi_b3p_enable(int on);
int gi_b3v_enable(int on);
/* gi_ggnn_forward / backward: their GI_GEMM_BF3 launches as fp16x2 (GI_GEMM_X2: two scaled fp16 planes per operand,
 * three products; environment GI_X2, default 1) or as bf16x3 (0).  on < 0 queries; returns the previous setting. */
int gi_x2_enable(int on);
/* Process-wide switch of gi_ggnn_forward / backward's use of GI_GEMM_BF3 launches (initial value: environment
 * GI_BF3, else GI_BF3_DEFAULT): on = 1 / 0 sets it, on < 0 only queries; returns the previous setting.  The
 * workspace size does not depend on it. */
int gi_bf3_enable(int on);
long long gi_bf3_image_elems(int rows, int cols);
int gi_bf3_pack(const gi_bf3_pack_desc* descs, int n, void* stream);

long long gi_mlp_chain_image_floats(const gi_chain_params* p);
int gi_mlp_chain_pack(const gi_chain_params* chains, int nchains, void* stream);
/* nchains (1 or 2, same direction) independent chains in one launch; `image` must be packed. */
int gi_mlp_chain(const gi_chain_params* chains, int nchains, void* stream);
/* Test / measurement hook (process-wide; the launcher's own choices are tile_rows = 0, rows64 = -1, ring = 2,
 * trace = NULL): tile_rows in 32..36 forces the row-block height (32 MFMA rows + extra rows on the VALU);
 * rows64 = 1 / 0 forces / forbids the 64-row variant (-1: where it pays); ring = 3 streams the weights of
 * 32-row blocks through a three-slot ring (146 KB of LDS; 2: two slots, 114 KB, a GEMM workgroup fits beside it);
 * trace = device buffer of 16 int64 per workgroup for per-phase timestamps (tools/trace_chain.py). */
int gi_mlp_chain_config(int tile_rows, int rows64, int ring, void* trace);

/* ------------------------------------------------------------------------------------------
 * Graph / pointwise kernels
 * ------------------------------------------------------------------------------------------ */
/* K4 seg_sum — replaces `torch.matmul(message_summation_matrix, message_terms)`
 * (gnn/summation_mpnn.py:141) and, in backward, the scatter of d(gathered rows):
 *   out[c, 0:cols] (+)= sum_{k in [off[c], off[c+1])} vals[perm[k], 0:cols],  c < rows */
int gi_seg_sum(const float* vals, int ldv, const int* perm, const int* off, int rows, int cols,
               float* out, int ldo, int accumulate, void* stream);

/* Backward of the aggregation onto MESSAGE rows, fused with the SELU backward of the message MLP's
 * last layer, in place:  y[u, c] = selu'(y[u, c]) * sum_{k in [off[u], off[u+1])} vals[perm[k], c] */
int gi_seg_sum_dselu(const float* vals, int ldv, const int* perm, const int* off, int rows, int cols,
                     float* y, int ldy, void* stream);

/* y[r, c] = selu'(y[r, c]) * sum_{s < nsplit} slabs[s * stride + r * ld + c]: sums the split-K slabs
 * of the pass-0 aggregation backward (cmat^T . d agg) with the SELU backward folded in. */
/* y_i[d, c] = selu'(y_i[d, c]) * sum_{k in [off[d], off[d+1])} vals_i[idx[k], c] for i = 0 (and 1 when
 * vals1 != NULL): the per-row sums of AttentionGGNN's pass-0 softmax backward (long segments). */
int gi_class_sum_dselu(const float* vals0, const float* vals1, int ldv, const int* idx, const int* off,
                       int rows, int cols, float* y0, float* y1, int ldy, void* stream);
int gi_slab_sum_dselu(const float* slabs, int nsplit, long long stride, int rows, int cols, int ld,
                      float* y, int ldy, void* stream);

/* out[r, c] = epilogue(sum_{s < nsplit} slabs[s * stride + r * ld + c]), epilogue = GI_EPI_* flags as in
 * gi_gemm (BIAS, SELU, DSELU / MULACT through act, ACCUM): finishes a GI_GEMM_SPLITK forward / dgrad
 * problem — the skinny, long-reduction layers of the graph-level stacks (B rows, K = N*A + G: 9 252 at the
 * ChEMBL shape) run split-K so that more than a handful of workgroups share the reduction. */
int gi_slab_epilogue(const float* slabs, int nsplit, long long stride, int rows, int cols, int ld,
                     int flags, const float* bias, const float* act, int ldact, float* out, int ldo,
                     void* stream);

/* Attention aggregation of AttentionGGNN — replaces `aggregate_message` (gnn/mpnn.py:370-389:
 * mask, Softmax(dim=1) over the padded neighbour axis, weighted sum) on the destination CSR:
 *   att[k, f] = softmax over k in [off[c], off[c+1]) of en[perm[k], f];
 *   out[c, f] = sum_k att[k, f] * emb[perm[k], f]        (0 for an empty segment),  c < rows.
 * en / emb: [U, ld] post-SELU outputs of the per-bond-type energy / message MLPs on message rows;
 * perm = in_perm (dst-CSR slot -> message row). */
int gi_seg_softmax_fwd(const float* en, const float* emb, int ld, const int* perm, const int* off,
                       int rows, int cols, float* out, int ldo, void* stream);
/* Its backward, per edge: with dagg = d loss / d out,
 *   d_emb_e[k, f] = att[k, f] * dagg[c, f],   d_en_e[k, f] = att[k, f] * (emb[perm[k], f] * dagg[c, f] - <att, emb*dagg>_c)
 * written in dst-CSR slot order [E, lde] (the softmax is recomputed from en).  The message-row
 * gradients are gi_seg_sum_dselu of these over the message CSR (perm = mu_slot, off = mu_off). */
int gi_seg_softmax_bwd(const float* en, const float* emb, int ld, const int* perm, const int* off,
                       int rows, int cols, const float* dagg, int ldd, float* d_en_e,
                       float* d_emb_e, int lde, void* stream);

/* out[r, c] = dY[idx ? idx[r] : r, c] * selu'(Y[r, c])  (may run in place on Y) */
int gi_selu_bwd_rows(const float* dY, int lddy, const int* idx, const float* Y, int ldy,
                     float* out, int ldo, int rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------
 * AlphaDropout, training mode with p > 0 — `torch.nn.AlphaDropout(dropout_p)` behind every
 * Linear + SELU of gnn/modules.py:130-142 (MLP._linear_block), including the last one.
 * ------------------------------------------------------------------------------------------
 * One site = one MLP layer's output buffer.  keep(row, col) is a counter-based hash of (seed, id,
 * row, col) compared with thresh = p * 2^32; nothing is stored except, `fshift` floats behind every
 * activation, the factor d y / d z = keep * a * selu'(z) the backward multiplies by
 * (GI_EPI_MULACT; the *_f variants below).  The arithmetic is ATen's _dropout_impl:
 *   y = fl(fl(s * (keep ? a : 0)) + (keep ? b_keep : b_drop)),  a = ((alpha'^2 p + 1)(1 - p))^-1/2,
 *   b = (keep - 1) * alpha' a + alpha' a p,  alpha' = 1.7580993408473766  (every scalar cast to fp32). */
typedef struct gi_dropout_params {
    unsigned long long seed;
    unsigned id, thresh;
    float a, b_keep, b_drop;
} gi_dropout_params;
/* fills `out` for probability p in [0, 1) (p == 0: keep everything, y == s, factor == selu') */
int gi_dropout_setup(double p, unsigned long long seed, unsigned id, gi_dropout_params* out);
/* in place on y[rows, 0:cols] (SELU outputs) -> AlphaDropout outputs; factors to y + fshift */
int gi_alpha_dropout_fwd(float* y, int ldy, int rows, int cols, long long fshift,
                         const gi_dropout_params* q, void* stream);
/* test hook: the keep bits of one site as bytes [rows, ld] */
int gi_dropout_mask(const gi_dropout_params* q, int rows, int cols, unsigned char* keep, int ld,
                    void* stream);
/* The SELU-backward sites with the factor read from `fshift` floats behind the activation instead of
 * derived from it (fshift == 0: exactly the functions without the suffix; fshift % 4 == 0). */
int gi_seg_sum_dselu_f(const float* vals, int ldv, const int* perm, const int* off, int rows,
                       int cols, float* y, int ldy, long long fshift, void* stream);
int gi_selu_bwd_rows_f(const float* dY, int lddy, const int* idx, const float* Y, int ldy,
                       float* out, int ldo, int rows, int cols, long long fshift, void* stream);
int gi_gather_readout_bwd_f(float* en, float* emb, int ld, const int* cidx, const int* node_mask,
                            int B, int N, int G, int S, float big,
                            const float* dg0, int ld0, const float* dg1, int ld1,
                            const float* dg2, int ld2, float* zpart, long long fshift, void* stream);
int gi_compress_slots_f(float* t1, int ldt, const int* cidx, int B, int N, int W, int S,
                        const float* dcat, int ldc, float* zpart, int ldz, long long fshift,
                        void* stream);

/* GRU gates — torch.nn.GRUCell as used at gnn/mpnn.py:249-253,296-297, applied only to rows
 * with >=1 incoming edge (gnn/summation_mpnn.py:107,124,143-144 update only those nodes).
 * In: gi,gh [rows,3H] (+bias already added), hx_prev [rows, ldh]; out: hx_new (cols [0,H) and
 * the feature tail [H,H+Fn) copied); gi is overwritten with (r|z|n), gh keeps W_hn h + b_hn. */
/* The whole GRU update of a message pass (torch.nn.GRUCell as called at gnn/mpnn.py:296-297, with the node mask of
 * gnn/summation_mpnn.py:146) in ONE launch: gi = agg W_ih^T + b_ih, gh = h W_hh^T + b_hh on the fp32 MFMA and the gate
 * arithmetic in registers.  agg [rows, lda] (M columns), hx [rows, ldh] = [h (H) | features | padding], W_ih [3H, M],
 * W_hh [3H, H] row-major.  Writes h' and the copied tail into hx_new [rows, ldh], and what gi_gru_gates_bwd reads: the
 * gates r, z, n into gi[:, 0:3H], gh_n into gh[:, 2H:3H] (gi / gh rows of nodes without incoming edges, and gh[:, 0:2H],
 * are left untouched).  H % 4 == M % 4 == lda % 4 == ldh % 4 == 0, 16-byte aligned agg / hx / hx_new; GI_EINVAL otherwise
 * (callers then use gi_gemm_batch + gi_gru_gates_fwd). */
int gi_gru_forward(const float* agg, int lda, const float* hx, int ldh, const float* Wih, const float* Whh,
                   const float* bih, const float* bhh, float* gi, float* gh, int ldg, float* hx_new,
                   const int* seg_off, int rows, int H, int M, void* stream);
int gi_gru_gates_fwd(float* gi, float* gh, int ldg, const float* hx_prev, float* hx_new, int ldh,
                     const int* seg_off, int rows, int H, int Fn, void* stream);
/* In: dh_new (+ up to three more partial gradients dh_b/c/d or NULL, all [rows, lddh]);
 * gi=(r|z|n), gh=(..|..|hn) from forward are overwritten with d gi, d gh;
 * dh_prev = direct part of the gradient to h_prev. */
int gi_gru_gates_bwd(float* gi, float* gh, int ldg, const float* hx_prev, int ldh,
                     const float* dh_new, const float* dh_b, const float* dh_c, const float* dh_d,
                     float* dh_prev, int lddh, const int* seg_off, int rows, int H, void* stream);

/* Launch-count reductions of the training step.  gi_fuse_flags() = the bit mask (environment GI_FUSE,
 * default GI_FUSE_DEFAULT) of the fused / vectorised variants gi_ggnn_forward / gi_ggnn_backward use.
 * DH_SCATTER, TIER2_DSELU and SLOTS reproduce the launches they replace bit for bit (same
 * operations, same summation orders; tests/test_kernels_gpu.py compares them with torch.equal); GATES_V4
 * evaluates the same formulas four hidden units at a time and agrees with the scalar kernels to rounding
 * (hipcc contracts the multiply-adds of the vector code differently: <= 1e-6 relative, same test file).
 *   GATES_V4     gi_gru_gates_fwd / _bwd on 16-byte vectors (4 hidden units per thread) when H % 4 == 0
 *   DH_SCATTER   the scatter of the message stacks' input gradients to their source nodes
 *                (gi_seg_sum over the source CSR, accumulating into d h; backward of
 *                `nodes[edge_batch_nghb_idc]`, gnn/summation_mpnn.py:131-133) folded into the
 *                gi_gru_gates_bwd_ex launch of the next (earlier) message pass
 *   TIER2_DSELU  the SELU backward of the three logit column ranges in one launch (gi_selu_bwd_cols3_f)
 *   SLOTS        fAddNet1 / fConnNet1 glue in one launch each way (gi_expand_slots2, gi_compress_slots2_f)
 * Every model kind follows the mask in both directions: the forward and the backward of GGNN, AttentionGGNN and MNN
 * share one driver.  (The MNN backward used to run the TIER2_DSELU and SLOTS launches whatever the mask said; with a
 * bit cleared it now runs the unfused launches, like the other kinds.  Nothing changes under the default mask.) */
#define GI_FUSE_GATES_V4    1
#define GI_FUSE_DH_SCATTER  2
#define GI_FUSE_TIER2_DSELU 4
#define GI_FUSE_SLOTS       8
/* Measured on the headline step (round 2, two A/B pairs): 15 -> 2.319 / 2.325 ms against 2.359 / 2.353 with
 * everything off. */
#define GI_FUSE_DEFAULT     15
int gi_fuse_flags(void);
/* gi_gru_gates_bwd with d h = dh_new + sum over the source-CSR segment [sc_off[r], sc_off[r+1]) of the rows
 * sc0[sc_perm[k]] (+ the same over sc1 when non-NULL; both [*, ldsc >= H]) — what gi_seg_sum(sc, sc_perm,
 * sc_off, ..., dh_new, accumulate) launches in front of gi_gru_gates_bwd would have left in dh_new, bit for
 * bit.  sc0 == NULL: plain gi_gru_gates_bwd on the vector kernel (scalar kernel when H % 4 != 0 or a
 * pointer / leading dimension is not 16-byte aligned; with sc0 that case is GI_EINVAL). */
int gi_gru_gates_bwd_ex(float* gi, float* gh, int ldg, const float* hx_prev, int ldh,
                        const float* dh_new, const float* dh_b, const float* dh_c, const float* dh_d,
                        float* dh_prev, int lddh, const int* seg_off, int rows, int H,
                        const float* sc0, const float* sc1, int ldsc, const int* sc_perm,
                        const int* sc_off, void* stream);
/* out_k[r, c] = dY[r, s_k + c] * selu'(Y[r, s_k + c]) for the three consecutive column ranges of widths
 * n0, n1, n2 (s_0 = 0, s_1 = n0, s_2 = n0 + n1): three gi_selu_bwd_rows_f calls in one launch
 * (backward entry of the tier-2 stacks, gnn/modules.py:265-279).  fshift as in gi_selu_bwd_rows_f. */
int gi_selu_bwd_cols3_f(const float* dY, int lddy, const float* Y, int ldy, long long fshift, int rows,
                        int n0, float* out0, int ld0, int n1, float* out1, int ld1,
                        int n2, float* out2, int ld2, void* stream);
/* gi_expand_slots for two tier-1 outputs (a, b) sharing cidx in one launch; gi_compress_slots_f likewise */
int gi_expand_slots2(const float* t1a, int ldta, int Wa, float* cata, int ldca,
                     const float* t1b, int ldtb, int Wb, float* catb, int ldcb,
                     const int* cidx, int B, int N, void* stream);
int gi_compress_slots2_f(float* t1a, int ldta, int Wa, const float* dcata, int ldca, float* zparta, int ldza,
                         float* t1b, int ldtb, int Wb, const float* dcatb, int ldcb, float* zpartb, int ldzb,
                         const int* cidx, int B, int N, int S, long long fshift, void* stream);

/* Small launches taken off the single-queue path of the training step.  gi_glue_flags() = the bit mask
 * in use: environment GI_GLUE, default GI_GLUE_DEFAULT; a word of its own, GI_FUSE and GI_FUSE_DEFAULT are unchanged.
 * gi_glue_set(mask) overrides it for the process (mask < 0: back to the environment's value) and returns the mask then
 * in use.  Every variant performs the floating-point operations of the launches it replaces in the same order: results
 * are bit for bit the same (tests/test_glue_gpu.py).
 *   READOUT_FWD  gi_gather_readout_fwd + gi_expand_slots2 of the GGNN / AttentionGGNN forward in one launch
 *   READOUT_BWD  gi_gather_readout_bwd_f + gi_compress_slots2_f of their backward in one launch
 *   LOSS_MEAN    the batch mean of the KL loss inside the row kernel's launch (gi_kl_loss_mean, loss.py); measured slower
 *                than the two launches it replaces and therefore not in the default
 *   GRU_AGG      GGNN passes >= 1: the sum of the incoming messages (gi_seg_sum) inside the fused GRU update's launch,
 *                where that launch has no more workgroups (64 rows x 64 hidden units) than the device has CUs */
#define GI_GLUE_READOUT_FWD 1
#define GI_GLUE_READOUT_BWD 2
#define GI_GLUE_LOSS_MEAN   4
#define GI_GLUE_GRU_AGG     8
/* Measured on the headline step (four rounds of alternating runs, profiles/glue/README.md): 11 -> 1.765 - 1.774 ms
 * against 1.779 - 1.788 for the parent. */
#define GI_GLUE_DEFAULT     11
int gi_glue_flags(void);
int gi_glue_set(int mask);
/* gi_gather_readout_fwd(en, ..., out2, ld2) and gi_expand_slots2(t1a, ..., catb, ldcb, cidx, B, N) in one launch: the
 * gather's workgroups followed by the expand's (the two read only tier-1 outputs and write disjoint memory). */
int gi_readout_glue_fwd(const float* en, const float* emb, int ld, const int* cidx, const int* node_mask,
                        int B, int N, int G, float big, float* out0, int ld0, float* out1, int ld1,
                        float* out2, int ld2, const float* t1a, int ldta, int Wa, float* cata, int ldca,
                        const float* t1b, int ldtb, int Wb, float* catb, int ldcb, void* stream);
/* gi_gather_readout_bwd_f(en, ..., zpart, fshift) and gi_compress_slots2_f(t1a, ..., zpartb, ldzb, cidx, B, N, S, fshift)
 * in one launch (disjoint rows, disjoint partial-sum buffers; the column sums stay with gi_colsum_multi). */
int gi_readout_glue_bwd_f(float* en, float* emb, int ld, const int* cidx, const int* node_mask, int B,
                          int N, int G, int S, float big, const float* dg0, int ld0, const float* dg1,
                          int ld1, const float* dg2, int ld2, float* zpart, float* t1a, int ldta, int Wa,
                          const float* dcata, int ldca, float* zparta, int ldza, float* t1b, int ldtb,
                          int Wb, const float* dcatb, int ldcb, float* zpartb, int ldzb, long long fshift,
                          void* stream);
/* gi_seg_sum(vals, ldv, perm, seg_off, rows, M, agg, lda, 0) followed by gi_gru_forward(agg, ...) in one launch: every
 * workgroup of the fused update first sums the incoming messages of its own 64 rows into LDS, in gi_seg_sum's order;
 * the workgroups of the first unit tile also write them to agg [rows, lda] (the backward reads it).  rows_dev (device
 * int, or NULL): min(rows, *rows_dev) rows are processed.  Conditions of gi_gru_forward, and ldv % 4 == 0, 16-byte
 * aligned vals; GI_EINVAL otherwise. */
int gi_gru_forward_agg(const float* vals, int ldv, const int* perm, float* agg, int lda, const float* hx, int ldh,
                       const float* Wih, const float* Whh, const float* bih, const float* bhh, float* gi, float* gh,
                       int ldg, float* hx_new, const int* seg_off, int rows, const int* rows_dev, int H, int M,
                       void* stream);

/* MNN message function, aggregate first (gnn/mpnn.py:58-63 + the sum of gnn/summation_mpnn.py:141):
 *   out[c, k * Fe + t] = sum over the dst-CSR slots s in [seg_off[c], seg_off[c+1]) whose message row u = in_perm[s]
 *                        has bond type t (type_off buckets) of h[u_src[u], k],     c < rows, k < H
 * (ldh % 4 == 0, ldh >= H rounded up to 4, 16-byte aligned h / out, ldo >= H * Fe; rows without in-edges get 0). */
int gi_typed_seg_sum(const float* h, int ldh, const int* u_src, const int* in_perm, const int* seg_off,
                     const int* type_off, int rows, int H, int Fe, float* out, int ldo, void* stream);
/* its transpose (backward onto the source rows):
 *   dh[c, k] (+)= sum over u in out_perm[src_off[c] .. src_off[c+1]) of sum over e in [mu_off[u], mu_off[u+1]) of
 *                 dS[mu_dst[e], k * Fe + type(u)]                                  c < rows, k < H */
int gi_typed_seg_sum_t(const float* dS, int lds, const int* out_perm, const int* src_off, const int* mu_off,
                       const int* mu_dst, const int* type_off, int rows, int H, int Fe, float* dh, int lddh,
                       int accumulate, void* stream);
/* MNN readout graph sum (gnn/mpnn.py:69-74): g[b, 0:H] = sum_{n < N} h[cidx[b*N + n], 0:H], written to up to three
 * destinations (NULL: skipped).  Backward: dh[c, 0:H] (+)= dg0[b] + dg1[b] + dg2[b] for every compact row c < S with
 * b = slot_of[c] / N; row S (the zero row shared by padded slots) is left alone when accumulating, else set to 0. */
int gi_graph_sum_fwd(const float* h, int ldh, const int* cidx, int B, int N, int H, float* out0, int ld0,
                     float* out1, int ld1, float* out2, int ld2, void* stream);
int gi_graph_sum_bwd(const float* dg0, int ld0, const float* dg1, int ld1, const float* dg2, int ld2,
                     const int* slot_of, int S, int N, int H, float* dh, int lddh, int accumulate, void* stream);

/* K7 gather readout — gnn/modules.py:44-52: g[b,:] = sum_n softmax_n(en[cidx[b,n]] - big*[mask==0]) * emb[cidx[b,n]],
 * written to up to three destinations (tier-2 concat inputs). */
int gi_gather_readout_fwd(const float* en, const float* emb, int ld, const int* cidx,
                          const int* node_mask, int B, int N, int G, float big,
                          float* out0, int ld0, float* out1, int ld1, float* out2, int ld2,
                          void* stream);
/* backward: dg = dg0+dg1+dg2 per graph; writes dZ of the last att/emb layers IN PLACE over
 * en/emb rows < S, and per-graph partial sums for the zero row into zpart[B, 2*G]. */
int gi_gather_readout_bwd(float* en, float* emb, int ld, const int* cidx, const int* node_mask,
                          int B, int N, int G, int S, float big,
                          const float* dg0, int ld0, const float* dg1, int ld1,
                          const float* dg2, int ld2, float* zpart, void* stream);

/* tier-1 -> tier-2 glue (gnn/modules.py:256-262 `view` + `cat`):
 *   cat[b, n*W + w] = t1[cidx[b,n], w] */
int gi_expand_slots(const float* t1, int ldt, const int* cidx, int B, int N, int W,
                    float* cat, int ldc, void* stream);
/* backward: t1 rows < S are overwritten in place with dcat * selu'(t1); inactive slots are
 * summed per graph into zpart[B, W] (raw, no selu'). */
int gi_compress_slots(float* t1, int ldt, const int* cidx, int B, int N, int W, int S,
                      const float* dcat, int ldc, float* zpart, int ldz, void* stream);
/* out[c] = (sum_b part[b, c]) * (y ? selu'(y[c]) : 1), deterministic */
int gi_colsum(const float* part, int ldp, int rows, int cols, const float* y, float* out,
              void* stream);
/* n (<= 8) independent column sums in one launch */
typedef struct gi_colsum_desc {
    const float* part; int ldp, rows, cols; const float* y; float* out;
} gi_colsum_desc;
int gi_colsum_multi(const gi_colsum_desc* descs, int n, void* stream);

/* sums wgrad slabs into the parameter gradients: for each descriptor,
 *   dW[n,k] = sum_s slab[s][n*ld + k] (k < K),  db[n] = sum_s slab[s][n*ld + K] */
typedef struct gi_reduce_desc {
    const float* slabs; float* dW; float* db;
    long long slab_stride; int n_slabs, N, K, ld;
} gi_reduce_desc;
int gi_reduce_slabs(const gi_reduce_desc* descs, int n_desc, void* stream);

/* torch.optim.Adam step (no amsgrad) over ONE flat fp32 bucket of n floats (n % 4 == 0, 16-byte
 * aligned): the optimizer the reference builds at Workflow.py:219-263, as a single launch. */
int gi_adam_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int step, void* stream);

/* Workflow.loss (Workflow.py:833-860) forward + gradient in one pass over the logits:
 * row_loss[b] = KL(target_b / sum(target_b) || softmax(out_b)); loss = mean_b row_loss[b];
 * d_out (may be NULL) = d loss / d out; loss_mean (may be NULL) = the scalar batch mean, summed in a
 * fixed order.  All-zero target rows give NaN like the reference. */
int gi_kl_loss(const float* out, int ldo, const void* target, int tgt_dtype, int ldt, int B,
               int width, float* row_loss, float* d_out, int ldd, float* loss_mean, void* stream);
/* The same in ONE launch (loss_mean required): the workgroup that finishes last sums the row losses, in the order of
 * gi_kl_loss's second launch — the same bits.  No workgroup waits for another.  The workgroups count themselves on a
 * word owned by the library, which the last one leaves zero again.  Each call takes the next word of a ring of 64 per
 * device; calls recorded into a graph use a second ring of 64, so a replayed graph never shares a word with an eager
 * call.  Limit: results are undefined when two launches on the same word run at the same time, that is with more than
 * 64 eager calls in flight on a device at once (on 65 or more streams), when more than 64 calls were recorded and two
 * graphs 64 recordings apart replay concurrently, or when ONE recorded call replays concurrently with itself. */
int gi_kl_loss_mean(const float* out, int ldo, const void* target, int tgt_dtype, int ldt, int B,
                    int width, float* row_loss, float* d_out, int ldd, float* loss_mean, void* stream);

/* Validation NLL of the correct actions, Analyzer.get_validation_likelihood (Analyzer.py:754-774), for one
 * batch in two launches with no host read-back.  Per row b of out [B, width] (row stride ldo) and target
 * [B, width] (GI_DTYPE, row stride ldt):
 *   s_b = sum_j (t_j / T) * softmax(out_b)_j,  T = sum_j t_j   (linear space, the reference's element order)
 * Rows whose s_b is NaN (T == 0, a NaN or +inf logit) are dropped; the others' -log(s_b) (+inf where s_b
 * underflows) go to dst[start + rank] in row order.  Entries past the kept rows keep their contents.
 * *n_structures += sum_b target[b, width-1] (every row, in a fixed order).  If the kept rows would run past
 * dst_len, the batch writes and counts nothing and sets *err = 1; while *err != 0 every call is a no-op.
 * ws: 2 B floats of workspace.  Deterministic (no atomics). */
int gi_eval_nll(const float* out, int ldo, const void* target, int tgt_dtype, int ldt, int B, int width,
                float* dst, long long dst_len, long long start, float* n_structures, int* err, float* ws,
                void* stream);

/* x[0:n] *= *scale with the scalar read on the device (the upstream gradient autograd hands to the
 * loss node: `loss.backward()` passes ones, RL-style callers pass a weight) — no host read-back. */
int gi_scale_by_scalar(float* x, long long n, const float* scale, void* stream);

/* Sampling step of graph generation — replaces `softmax(model(nodes, edges))` +
 * GraphGenerator.get_actions / get_invalid_actions (GraphGenerator.py:121, 467-657) with one launch:
 * per graph b, softmax of logits[b, 0:W] (W = N*A + N*Fe + 1), ONE categorical draw = the first
 * action whose cumulative probability exceeds uniform[b] (inverse CDF; uniform in [0,1]), decode and
 * validity rules.  Only actions of positive fp32 probability are drawn; u = 1 draws the last of them.  n_nodes[B] int32 = atoms currently in each graph; edges [B,N,N,Fe] (GI_DTYPE).
 *   action[b] = {kind (0 add, 1 connect, 2 terminate), node_to, rem, from}: rem = index inside the
 *               node's block (add: ravelled (atom type, charge, ..., bond type); connect: bond type);
 *               from = n_nodes (add; 0 where the reference resets it, :567) or n_nodes-1 (connect)
 *   likelihood[b] = probability of the drawn action (:541)
 *   flags[b]  bit 0: invalid action (:573-646); bit 1: the add's "connect to" index was reset (:650-654) */
int gi_sample_actions(const float* logits, int ldl, const float* uniform, const int* n_nodes,
                      const void* edges, int edges_dtype, int B, int N, int A, int Fe, int* action,
                      float* likelihood, int* flags, void* stream);

/* Sampling step of RL fine-tuning — replaces `softmax(agent(...))`, `softmax(prior(...))` +
 * GraphGeneratorRL.get_actions / get_invalid_actions (GraphGeneratorRL.py:131-135, 521-720): the
 * draw, decode and validity rules of gi_sample_actions on the agent's logits (action, like_agent and
 * flags are bit-identical to gi_sample_actions for the same agent row and uniform), plus
 *   like_prior[b] = softmax(prior_logits[b])[drawn index]
 *   idx[b]        = the drawn flat index;  lse[2b + 0 / 1] = log-sum-exp of the agent / prior row
 * (the state gi_sample_likelihood_bwd needs).  lda / ldp: row pitches of the two logits matrices. */
int gi_sample_actions_rl(const float* agent_logits, int lda, const float* prior_logits, int ldp,
                         const float* uniform, const int* n_nodes, const void* edges,
                         int edges_dtype, int B, int N, int A, int Fe, int* action,
                         float* like_agent, float* like_prior, int* flags, int* idx, float* lse,
                         void* stream);

/* Backward of the two likelihoods of gi_sample_actions_rl (softmax Jacobian at the drawn index):
 *   d[b, j] = g[b] * like[b] * (delta(j, idx[b]) - exp(logits[b, j] - lse[b, side]))
 * for the agent (side 0) and the prior (side 1) in one launch; a side whose g is NULL is skipped.
 * d_agent / d_prior are written (not accumulated), W <= the sampler's row limit (GI_ELIMIT). */
int gi_sample_likelihood_bwd(int B, int W, const int* idx, const float* lse,
                             const float* agent_logits, int lda, const float* g_agent,
                             const float* like_agent, float* d_agent, int ldda,
                             const float* prior_logits, int ldp, const float* g_prior,
                             const float* like_prior, float* d_prior, int lddp, void* stream);

/* Growth step of graph generation — the bookkeeping of one GraphGenerator.build_graphs round after the draw
 * (GraphGenerator.py:126-157 with copy_terminated_graphs :340-387, apply_actions :211-338 and reset_graphs
 * :430-465), in place on the generator's own tensors, from gi_sample_actions' raw action / likelihood / flags
 * (no index tuples, no read-back).  Let n = state[0] (graphs generated so far), r = state[1] (round) at entry:
 *   - frozen: nothing at all when n >= state[2] (target = batch_size) or state[3] (error) != 0;
 *   - T = graphs with kind == 2 (graph 0 included), I = graphs with flags & 1, both ascending;
 *     S = (T without 0) followed by (I without 0) (:130-133); properly_terminated[n : n + |T|] = 1 (:127, clipped at C);
 *   - graph S[k] is copied to generated row n + k: nodes, edges, n_nodes and its likelihood row with
 *     likelihoods[g, r] = likelihood[g] (:365-383);
 *   - every graph's action is applied (:211-338: graph 0's and the terminated ones' too): add sets
 *     nodes[g, from, off_j + sub_j] = 1 per node-feature group j (rem unravelled over group[] then Fe), both edge
 *     directions of bond type rem % Fe unless n_nodes[g] was 0, n_nodes[g] += 1; connect sets both directions (from = -1
 *     wraps to N - 1); both write likelihoods[g, r]; terminate does nothing;
 *   - S is reset (zeros, :430-465), graph 0 restored (nodes[0] = 1, edges[0,0,0,0] = 1, n_nodes[0] = 1; its other
 *     edges stay), then state[0] += |S|, state[1] += 1.
 * Every index is checked before any write of the round.  Where the reference raises, the round writes nothing and
 * OR-s a GI_GROW_ERR_* bit into state[3], which freezes every later round.  state = GI_GROW_STATE_WORDS + B ints of
 * device memory (gi_grow_state_words), zero-filled with state[2] = target before the first round; host_state = NULL
 * or 4 ints of mapped host memory (gi_host_flag_create) that receive state[0..3] at the end of every round.
 * Three launches in stream order (scan and validate / per-graph copy, apply, reset / counters). */
#define GI_GROW_MAX_GROUPS 8
#define GI_GROW_STATE_WORDS 16
#define GI_GROW_ERR_ROUND    1   /* r >= L: IndexError at the round's first likelihood write (:365, :305, :330) */
#define GI_GROW_ERR_CAPACITY 2   /* n + |S| > C: the slice assignment of :379-382 fails */
#define GI_GROW_ERR_ACTION   4   /* kind / node_to / rem / from out of range, or a graph both terminated and invalid */
#define GI_GROW_ERR_NNODES   8   /* n_nodes would overflow int8 */
typedef struct gi_grow_desc {
    float* nodes;                  /* [B, N, Fn] */
    float* edges;                  /* [B, N, N, Fe] */
    signed char* n_nodes;          /* [B] */
    float* likelihoods;            /* [B, L] */
    float* gen_nodes;              /* [C, N, Fn] */
    float* gen_edges;              /* [C, N, N, Fe] */
    signed char* gen_n_nodes;      /* [C] */
    float* gen_likelihoods;        /* [C, L] */
    signed char* properly_terminated;  /* [C] */
    const int* action;             /* [B, 4] of gi_sample_actions */
    const float* likelihood;       /* [B] */
    const int* flags;              /* [B] */
    int* state;                    /* device, gi_grow_state_words(B) ints */
    int* host_state;               /* NULL or mapped host memory, 4 ints */
    int B, N, Fn, Fe, L, C;
    int n_groups;                  /* node-feature groups of the add action (dim_f_add[1:-1]); sum(group) == Fn */
    int group[GI_GROW_MAX_GROUPS];
} gi_grow_desc;
int gi_grow_state_words(int B);
int gi_grow_graphs(const gi_grow_desc* desc, void* stream);

/* Growth step of RL fine-tuning — one GraphGeneratorRL.build_graphs round after the draw (GraphGeneratorRL.py:109-172
 * with apply_actions :227-380, copy_terminated_graphs :382-421 and reset_graphs :476-520), from
 * gi_sample_actions_rl's action / like_agent / like_prior / flags.  base is gi_grow_graphs' descriptor with
 * likelihoods / gen_likelihoods / likelihood = the agent's agent_likelihoods [B, L] / generated_agent_likelihoods
 * [C, L] / like_agent [B]; the round is gi_grow_graphs' (same launches, slots, properly_terminated, dummy graph 0,
 * error bits and freeze) with, in addition:
 *   - the prior stream (prior_likelihoods, gen_prior_likelihoods, prior_likelihood: all three set or all NULL) gets
 *     what the agent's does: written at column r by every applied add / connect and by the copy of S, copied to the
 *     generated row, reset for S;
 *   - start[g] = state[GI_GROW_STATE_WORDS + B + g] is the round in which graph g's current row began: 0 at first,
 *     r + 1 after g is reset in round r;
 *   - traj (NULL or [3, C] ints): the copy of graph g in round r to generated row k writes traj[k] = g,
 *     traj[C + k] = start[g], traj[2 C + k] = r.  Every graph other than 0 writes column r in every applied round
 *     (its add or connect, or the copy of S) and a reset zeroes the whole row, so generated row k holds
 *     like_c[traj[k]] (the round-c likelihood) at columns traj[C + k] .. traj[2 C + k] and 0 elsewhere.
 * state = gi_grow_rl_state_words(B) ints (GI_GROW_STATE_WORDS + 2 B), zero-filled with state[2] = target. */
typedef struct gi_grow_rl_desc {
    gi_grow_desc base;                 /* the agent's stream and everything else */
    float* prior_likelihoods;          /* [B, L] or NULL */
    float* gen_prior_likelihoods;      /* [C, L] or NULL */
    const float* prior_likelihood;     /* [B] or NULL (like_prior of gi_sample_actions_rl) */
    int* traj;                         /* [3, C] or NULL: source graph, first and last round of each generated row */
} gi_grow_rl_desc;
int gi_grow_rl_state_words(int B);
int gi_grow_graphs_rl(const gi_grow_rl_desc* desc, void* stream);

/* Seeded generation — the growth step with a bank of S >= 1 seed molecules (scaffolds) in the loader's int8 molecule
 * format, from which every graph starts and restarts instead of from the empty graph.  The bank is tightly packed
 * (seed s begins at byte s * N * Fn of nodes, s * N * N * Fe of edges): nothing is assumed of its alignment beyond
 * the base pointers, and the kernels read it one byte per element.  The caller guarantees what routes.check verifies:
 * 0 / 1 entries, n_nodes[s] in [0, N] equal to the number of non-padding node rows, nodes in a valid decoding order.
 *   - gi_grow_seed_init writes the first fill: slot 0 stays the dummy graph; slot g >= 1 takes seed (g - 1) mod S —
 *     nodes and edges converted to fp32, n_nodes set, its likelihood row (and the row of prior_likelihoods [B, L] when
 *     that is not NULL) zeroed.  Of desc it reads nodes, edges, n_nodes, likelihoods, state and B, N, Fn, Fe, L.
 *   - seed[g] = state[GI_GROW_STATE_WORDS + 2 B + g] is the seed slot g currently grows from (-1 for slot 0).
 *     state = gi_grow_seeded_state_words(B) = GI_GROW_STATE_WORDS + 3 B ints, for both seeded steps; every word
 *     of gi_grow_graphs / gi_grow_graphs_rl keeps its meaning (the start rounds stay at + B), zero-filled with
 *     state[2] = target before gi_grow_seed_init.
 *   - gi_grow_graphs_seeded / gi_grow_graphs_rl_seeded are gi_grow_graphs / gi_grow_graphs_rl (same three launches,
 *     slots, freeze after the target or an error, dummy graph's restore, host mirror, trajectory record, error bits)
 *     except that graph S[k], copied to generated row `row` = n + k, is reset to seed (B - 1 + row) mod S instead of
 *     to zeros, gen_seed[row] (when not NULL) receives seed[g], and seed[g] becomes the new seed.  No counter is
 *     added: the choice is a function of the row alone, deterministic and round-robin over the bank (the first fill
 *     uses seeds 0 .. B - 2, row 0 continues with B - 1); shuffle the bank to randomise.  The likelihood rows are
 *     reset to zeros as before.
 * A generated likelihood row holds only the actions sampled after the slot's (re)start: it is the likelihood of the
 * COMPLETION given the seed, not of the whole molecule.  The empty seed (n_nodes = 0, all bytes zero) is legal and
 * behaves exactly like the unseeded reset; a seed with n_nodes = N is legal too: the sampler's validity rules then
 * leave only connect and terminate. */
typedef struct gi_grow_seed_desc {
    const signed char* nodes;      /* [S, N, Fn] int8, device */
    const signed char* edges;      /* [S, N, N, Fe] */
    const signed char* n_nodes;    /* [S] */
    int* gen_seed;                 /* [C] or NULL: the seed each generated row was grown from */
    int S;
} gi_grow_seed_desc;
int gi_grow_seeded_state_words(int B);
int gi_grow_seed_init(const gi_grow_desc* desc, const gi_grow_seed_desc* seeds, float* prior_likelihoods,
                      void* stream);
int gi_grow_graphs_seeded(const gi_grow_desc* desc, const gi_grow_seed_desc* seeds, void* stream);
int gi_grow_graphs_rl_seeded(const gi_grow_rl_desc* desc, const gi_grow_seed_desc* seeds, void* stream);

/* The generated likelihood rows of a finished RL loop from the per-round likelihoods, and the backward of that map;
 * both sides (agent a, prior p) in one launch each, a side with NULL pointers skipped.  like_* are [R, B] (row c =
 * round c's like_agent / like_prior), traj is the [3, C] record of gi_grow_graphs_rl, n = rows generated.
 *   gather:  gen[k, c] = like[c, traj[k]] for k < n and traj[C + k] <= c <= traj[2 C + k] (c < R), 0 elsewhere of
 *            gen [C, L] (bit-identical to what gi_grow_graphs_rl wrote into gen_likelihoods);
 *   scatter: d_like[c, traj[k]] = g[k * ldg + c] on the same index set, 0 elsewhere of d_like [R, B].  No two rows
 *            share a (c, graph) pair: no atomics, every element written once. */
int gi_grow_traj_gather(int n, int R, int B, int C, int L, const int* traj, const float* like_a,
                        const float* like_p, float* gen_a, float* gen_p, void* stream);
int gi_grow_traj_scatter(int n, int R, int B, int C, int L, const int* traj, const float* g_a, int ldg_a,
                         const float* g_p, int ldg_p, float* d_a, float* d_p, void* stream);

/* Optional per-launch timing for the benchmark's roofline leg: when enabled, every gi_gemm and
 * gi_seg_sum launch is bracketed by hipEvents on its stream.  gi_prof_collect blocks until the
 * recorded work finished and returns, per kernel family k (0 = GEMM, 1 = seg_sum): summed elapsed
 * ms, busy ms = length of the UNION of the launches' [start, stop] intervals (launches on the
 * backward's two streams overlap; the sum double-counts that time), summed work (GEMM: useful flops
 * 2*M*N*K; seg_sum: 0, the caller knows the bytes) and the number of launches; it clears the log. */
int gi_prof_enable(int on);
int gi_prof_collect(double* ms, double* busy_ms, double* work, int* launches);
/* The GEMM family of the LAST gi_prof_collect split by the matrix pipe the launch ran on — [0] fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), [1] bf16 MFMA (GI_GEMM_BF3: six bf16 products per fp32 product), [2] f16 MFMA (GI_GEMM_X2:
 * three f16 products): summed elapsed ms, useful flops 2*M*N*K and launches, three entries each. */
int gi_prof_pipes(double* ms, double* work, int* launches);

/* ------------------------------------------------------------------------------------------
 * Whole-model entry points: one call enqueues the complete GGNN forward (or backward) —
 * `SummationMPNN.forward` message passes + `GGNN.readout` (gnn/summation_mpnn.py:128-149,
 * gnn/mpnn.py:284-303).  Parameters are passed as a pointer table in state_dict order.
 * ------------------------------------------------------------------------------------------ */
typedef struct gi_ggnn_dims {
    int B, N, Fn, Fe, H, M, G, A, C, passes;
    int enn_depth, enn_hidden, att_depth, att_hidden, emb_depth, emb_hidden;
    int mlp1_depth, mlp1_hidden, mlp2_depth, mlp2_hidden;
    float big_positive;
    /* model kind: GI_KIND_GGNN — sum aggregation (gnn/mpnn.py:229-303);  GI_KIND_ATTGGNN —
     * `AttentionGGNN` (gnn/mpnn.py:306-398): a second per-bond-type MLP (eatt_depth/eatt_hidden =
     * constants.att_depth / att_hidden_dim; enn_* then carry msg_depth / msg_hidden_dim) gives
     * attention energies, aggregated with gi_seg_softmax_*.  Parameter table order: msg_nns of all
     * bond types, [att_nns of all bond types,] gru, gather, APDReadout (state_dict order). */
    int kind, eatt_depth, eatt_hidden;
    /* AlphaDropout training mode (gnn/modules.py:130-142 with dropout_p > 0; eval and p == 0: all
     * zero).  dropout != 0: every MLP layer output goes through torch.nn.AlphaDropout with its
     * stack's probability (enn/msg stacks, AttentionGGNN's energy stacks, gather att_nn / emb_nn,
     * fAddNet1+fConnNet1, the three tier-2 stacks) and masks drawn from drop_seed.  Requires a graph
     * compacted WITHOUT row sharing (gi_compact_count_ex, nodedup = 1); the workspace doubles (every
     * activation gets a factor twin); the logits buffer `out` must have 2 B rows (rows [B, 2B) take
     * the factors of the logits) and the same buffer must be handed to the backward as y_out. */
    int dropout;
    float drop_enn, drop_eatt, drop_att, drop_emb, drop_mlp1, drop_mlp2;
    unsigned long long drop_seed;
} gi_ggnn_dims;
#define GI_KIND_GGNN 0
#define GI_KIND_ATTGGNN 1
/* GI_KIND_MNN — `MNN` (gnn/mpnn.py:16-74): message m(i <- j) = (sum_f e_f W[:, :, f]) h_j with ONE parameter
 * message_weights [M, H, Fe] (no per-bond-type MLPs), the same GRU update, and a readout that feeds the plain sum of
 * every slot's hidden state (graph_emb[b] = sum_n h[b, n], no gather stacks) to GlobalReadout.  G must equal H; every
 * depth other than mlp1_depth / mlp2_depth is 0.  Parameter table order: message_weights, gru, APDReadout.  Computed
 * aggregate-first: S_p = gi_typed_seg_sum of h, messages = S_p . W.view(M, H Fe)^T (gi_gemm).  No pass-0 row cache
 * (gi_p0_cache_words = 0, gi_graph.p0_cache ignored). */
#define GI_KIND_MNN 2

/* Creates / destroys a lowest-priority, non-blocking stream on the current device for
 * gi_ggnn_backward's `side_stream` argument (caller-owned handle; any other stream of the same
 * device works too). */
int gi_side_stream_create(void** stream);
int gi_side_stream_destroy(void* stream);

/* Number of parameter tensors of the model, or GI_ELIMIT past a compiled-in limit: every stack depth 0..11 (at most 12
 * Linear layers), 0..16 message passes, N <= GI_MAX_NODES, Fe <= GI_MAX_GROUPS. */
int gi_ggnn_num_params(const gi_ggnn_dims* d);
/* S active slots, E directed edges, U message rows, D0 pass-0 rows (counts[0], [1], [3], [20]) */
long long gi_ggnn_workspace_floats(const gi_ggnn_dims* d, int S, int E, int U, int D0);
long long gi_ggnn_slab_floats(const gi_ggnn_dims* d, int S, int U, const int* Ut);
/* ws must hold hx0 (from gi_compact_fill) at offset gi_ggnn_hx0_offset(); forward keeps every
 * activation in ws for backward. */
long long gi_ggnn_hx0_offset(const gi_ggnn_dims* d, int S, int E, int U, int D0);
int gi_ggnn_ldhx(const gi_ggnn_dims* d);
/* test/debug hook: offset (floats) and leading dimension of a named workspace buffer
 * ("hx" i=pass, "eact" i=pass j=layer, "m","agg","gi","gh" i=pass, "att_act" j=layer, "en", ...;
 * MNN: "ssum" i=pass — the typed sums S_p [R, H * Fe]) */
int gi_ggnn_ws_query(const gi_ggnn_dims* d, int S, int E, int U, int D0, const char* name, int i,
                     int j, long long* off, int* ld);
int gi_ggnn_forward(const gi_ggnn_dims* d, const float* const* params, const gi_graph* g,
                    float* ws, float* out, int ldout, void* stream);
/* The same with a second stream and run flags.  side_stream (may be NULL; gi_side_stream_create): everything that
 * depends on the WEIGHTS only is enqueued there instead of in front of the kernels that wait for it — the amax cells
 * of the fp16x2 layers' weights and their dynamic-range check (needed by the readout, ~0.4 ms into the forward), and,
 * with GI_RUN_PREPACK_BWD, what gi_ggnn_backward would otherwise pack at its start: the W^T images of the 16-bit-pipe
 * layers and the dZ chains' weight image (then call the backward with GI_BWD_PREPACKED: it waits for that work
 * instead of redoing it).  `stream` waits for the side stream where it needs the results, and at the end of the call
 * for the packs into `ws`: everything the caller enqueues on `stream` afterwards (the backward, a reuse of the
 * workspace's memory) is ordered behind the side stream's work on `ws`.
 * GI_RUN_NO_X2: this call's 16-bit-pipe launches as bf16x3 instead of fp16x2 (what GI_X2=0 does process-wide) — what a
 * caller switches to after gi_graph.x2_guard_host tripped.  Forward and backward of one tape must agree. */
#define GI_RUN_PREPACK_BWD 1
#define GI_RUN_NO_X2 2
int gi_ggnn_forward_ex(const gi_ggnn_dims* d, const float* const* params, const gi_graph* g,
                       float* ws, float* out, int ldout, void* stream, void* side_stream, int flags);
/* Pass-0 row cache for inference loops (generation: GraphGenerator.py:118-157 calls the model thousands of
 * times with the same weights).  In the first message pass h = [x | 0], so a message row (and AttentionGGNN's
 * energy row) depends only on (bond type, 0/1 feature pattern of the source node) and the weights: a few dozen
 * distinct rows per batch, the same ones forward after forward.  With gi_graph.p0_cache set, gi_ggnn_forward
 * looks every pass-0 row of the batch up in a device-side table keyed by (bond type, pattern); when all are
 * there, the rows are copied from the table and the pass-0 stack launch exits at once (gi_chain_params.
 * skip_flag), otherwise the stack runs as usual and its rows are added to the table (the table is emptied when
 * they would not fit).  No host involvement: works inside a bounded (host-sync-free) forward and a captured
 * hipGraph.  The CALLER zero-fills the buffer whenever a weight of the message / energy stacks changes
 * (gnn/mpnn.py does, from the parameters' versions).  words[0] = hit flag of the latest forward, [1] = rows
 * in the table, [2] / [3] = forwards / hits so far.  Returns the buffer size in 4-byte words, < 0 on error. */
long long gi_p0_cache_words(const gi_ggnn_dims* d);
/* floats of gi_graph.wcache for this model (independent of the batch) */
long long gi_ggnn_wcache_floats(const gi_ggnn_dims* d);
/* consumes (overwrites) the activations in ws; y_out = the logits forward returned; grads[i]
 * receives the gradient of params[i]; slabs = gi_ggnn_slab_floats() floats of scratch.
 * side_stream (may be NULL): a second hipStream_t of the same device.  When given, the weight-
 * gradient GEMMs run there, ordered after their operands by events, concurrently with the dZ chain
 * on `stream`; `stream` waits for them before the final slab reduction, so on return every piece of
 * work is ordered before whatever the caller enqueues next on `stream`. */
int gi_ggnn_backward(const gi_ggnn_dims* d, const float* const* params, const gi_graph* g,
                     float* ws, float* slabs, const float* y_out, int ldout, const float* d_out,
                     int lddout, float* const* grads, void* stream, void* side_stream);
/* The same in two calls, for overlapping the data-parallel gradient exchange with the backward:
 * GI_BWD_READOUT differentiates the readout (gather + APDReadout: ~86 % of the parameters) and
 * completes the gradients of params[gi_ggnn_first_readout_param() ..) — on `side_stream` when given
 * (record an event there to know when), else on `stream`; GI_BWD_PASSES then differentiates the
 * message passes and completes the rest.  Same arguments to both calls; GI_BWD_ALL = gi_ggnn_backward. */
#define GI_BWD_ALL 0
#define GI_BWD_READOUT 1
#define GI_BWD_PASSES 2
/* OR-ed into `phase`: GI_BWD_PREPACKED — the forward ran as gi_ggnn_forward_ex(.., GI_RUN_PREPACK_BWD) with the same
 * side stream: the weight images of this backward are (being) written there, the call waits for them instead of packing;
 * GI_BWD_NO_X2 — bf16x3 instead of fp16x2, like GI_RUN_NO_X2 (the forward of the same tape must have run that way). */
#define GI_BWD_PREPACKED 0x100
#define GI_BWD_NO_X2 0x200
int gi_ggnn_backward_phase(const gi_ggnn_dims* d, const float* const* params, const gi_graph* g,
                           float* ws, float* slabs, const float* y_out, int ldout,
                           const float* d_out, int lddout, float* const* grads, void* stream,
                           void* side_stream, int phase);
int gi_ggnn_first_readout_param(const gi_ggnn_dims* d);

/* ------------------------------------------------------------------------------------------
 * Decoding routes (gi_route.hip): from M whole molecules to the training rows the reference's preprocessing writes,
 * `PreprocessingGraph.get_decoding_route_state(k)` for k = 0 .. n_edges + 1 (MolecularGraph.py:691-732: k = 0 the
 * whole molecule with APD = terminate, k >= 1 the APD before the k-th `truncate_graph` and the graph after it), and
 * the merge of byte-identical subgraphs `DataProcesser.get_subgraphs` intends (DataProcesser.py:204-231).
 *
 * nodes [M, N, Fn] and edges [M, N, N, Fe] are int8, 0 / 1, nodes in the reference's order (every node i > 0 has a
 * lower neighbour), zero padded; a node's feature row is one-hot in each of the n_seg consecutive segments of sizes
 * seg[] (atom type, formal charge, then implicit Hs and chirality when configured; util.py:26-47), which are the
 * middle dimensions of dim_f_add = [N, seg.., Fe]; apd_width = N prod(seg) Fe + N Fe + 1 (GI_EINVAL otherwise).
 * Limits: N <= GI_MAX_NODES, Fe <= GI_MAX_GROUPS (GI_ELIMIT).
 *
 * counts[GI_ROUTE_COUNTS] int32 (device): [0] OR of the error bits of all molecules, [1] rows of the call (the sum of
 * the route lengths), [2] rows after the merge.  A molecule that violates the contract gets route length 0 and its
 * GI_ROUTE_ERR_* bits in mol_err[m]; it contributes no rows, nothing faults and nothing is written out of bounds.
 *
 *   gi_route_plan    zeroes counts; lengths[M] = n_edges + 2 (0 if invalid), mol_err[M], counts[0..1]; the per-pair
 *                    deletion steps and row offsets stay in plan_ws (gi_route_plan_ws_bytes).
 *   gi_route_expand  rows [0, min(counts[1], rows_cap)) in molecule-major, step-minor order: out_nodes
 *                    [rows_cap, N, Fn] and out_edges [rows_cap, N, N, Fe] int8; out_apd [rows_cap, apd_width] one-hot,
 *                    GI_DTYPE_I8 or GI_DTYPE_F32 (NULL: not written); row_mol / row_step [rows_cap] int32 (-1 past the
 *                    real rows, whose outputs are zero).  Every out_* buffer is written in whole aligned 16-byte
 *                    pieces: it must be 16-byte aligned and its size rounded up to 16 bytes.  Also leaves each row's
 *                    hot APD index and 64-bit content hash (AND hash_mask — ~0 in production; tests force collisions
 *                    with fewer bits) in rows_ws (gi_route_rows_ws_bytes(rows_cap, merge)).
 *   gi_route_merge   after gi_route_expand with the same rows_ws (allocated with merge = 1) and rows_cap, on its
 *                    out_nodes / out_edges / row_mol / row_step: rows with identical bytes become one row at the place
 *                    of their first occurrence, order kept; out_apd = the sum of their one-hot APDs (GI_DTYPE_I8 only
 *                    for M <= 127, a sum may reach M); out_row_mol / out_row_step name the first occurrence;
 *                    counts[2] = rows kept.  Same buffer sizes as gi_route_expand; rows past counts[2] are zero in
 *                    out_nodes / out_edges / out_apd.  Rows are grouped by hash and confirmed by a byte compare; the
 *                    result does not depend on launch timing (the sums are integer). */
#define GI_ROUTE_COUNTS 4
#define GI_ROUTE_ERR_VALUE 1        /* an entry of nodes or edges is not 0 / 1 */
#define GI_ROUTE_ERR_ONEHOT 2       /* a node's feature row is not one-hot in every segment */
#define GI_ROUTE_ERR_ASYMMETRIC 4   /* edges[i, j] != edges[j, i] */
#define GI_ROUTE_ERR_MULTI_BOND 8   /* several bond types on one pair */
#define GI_ROUTE_ERR_CONNECT 16     /* a node i > 0 without a neighbour of lower index */
#define GI_ROUTE_ERR_PADDING 32     /* nodes are not a zero-padded prefix, or a bond touches padding or the diagonal */
#define GI_ROUTE_ERR_EMPTY 64       /* no node at all */
typedef struct {
    int M, N, Fn, Fe;
    int n_seg, seg[4];
    int apd_width;
} gi_route_dims;
long long gi_route_plan_ws_bytes(const gi_route_dims* d);
long long gi_route_rows_ws_bytes(int rows_cap, int merge);
int gi_route_plan(const gi_route_dims* d, const signed char* nodes, const signed char* edges, void* plan_ws,
                  int* lengths, int* mol_err, int* counts, void* stream);
int gi_route_expand(const gi_route_dims* d, const signed char* nodes, const void* plan_ws, void* rows_ws,
                    const int* counts, int rows_cap, unsigned long long hash_mask, signed char* out_nodes,
                    signed char* out_edges, void* out_apd, int apd_dtype, int* row_mol, int* row_step, void* stream);
int gi_route_merge(const gi_route_dims* d, void* rows_ws, int* counts, int rows_cap, const signed char* in_nodes,
                   const signed char* in_edges, const int* in_row_mol, const int* in_row_step,
                   signed char* out_nodes, signed char* out_edges, void* out_apd, int apd_dtype, int* out_row_mol,
                   int* out_row_step, void* stream);

/* gi_route_rows_hot: *hot = the device pointer, inside the rows_ws of a gi_route_expand call with this rows_cap
 * (whatever `merge` it was allocated with), of hot[rows_cap] int32: the hot APD index of every unmerged row (apd_width
 * - 1 in the rows past the real ones, which row_mol marks with -1).  With out_apd = NULL this is all a likelihood
 * needs of the APDs.  Host arithmetic only. */
int gi_route_rows_hot(void* rows_ws, int rows_cap, int** hot);

/* ------------------------------------------------------------------------------------------
 * Log-likelihood of whole molecules along their decoding routes (gi_loglik.hip).  For route row r with logits z_r [W]
 * and hot APD index a_r:  row_ll[r] = z_r[a_r] - logsumexp(z_r);  mol_ll[m] = the sum over the rows of molecule m.
 * That is the log of the product over the route of the per-row probability of Analyzer.py:754-774 with a one-hot
 * target; it is evaluated in log space with the row maximum subtracted, so it stays finite where the reference's
 * linear-space product underflows.
 *
 * logits [rows, W] fp32 with row pitch ld >= W floats, W >= 1 without an upper limit; hot [rows] int32.  err: one int32
 * word on the device, OR-ed with GI_LL_ERR_* bits, never cleared here.
 *
 * gi_row_loglik      row_ll[r] and row_lse[r] = logsumexp(z_r); each row is read once.  hot[r] == -1 (a padding row):
 *                    nothing is read, both are 0.  hot[r] outside [-1, W): GI_LL_ERR_HOT, nothing is indexed with it
 *                    and the row's outputs are not written.  A NaN logit gives NaN; hot's logit -inf gives -inf.
 * gi_row_loglik_bwd  d_logits[r, j] = g_r (delta(j, hot[r]) - exp(z[r, j] - row_lse[r])), written, not accumulated
 *                    (row pitch ldd >= W); an entry whose logit is -inf gets exactly 0.  g_r = g_mol[row_mol[r]], plus
 *                    g_kind[row_mol[r], kind_r] when g_kind [n_mol, 3] is given (kind_r: hot < n_add -> 0, hot < n_add
 *                    + n_conn -> 1, else 2; n_add + n_conn + 1 == W); row_mol = NULL: g_r = g_mol[r].  Rows with hot
 *                    == -1 or row_mol == -1 are exactly zero; so are rows whose hot is outside [-1, W) (GI_LL_ERR_HOT)
 *                    or whose row_mol is outside [-1, n_mol) (GI_LL_ERR_MOL).
 * gi_mol_loglik_sum  mol_ll[m] += the sum of row_ll over the rows of the call with row_mol == m (-1: skipped), added
 *                    one by one in row order by one thread per molecule (no atomics): splitting the rows over several
 *                    calls in stream order, anywhere, gives the same bits as one call.  mol_kind [n_mol, 3] (NULL: not
 *                    wanted; needs hot, W, n_add, n_conn as above) += the same sum split by kind_r.  Contract: row_mol
 *                    is in [-1, n_mol) (GI_LL_ERR_MOL otherwise) and non-decreasing over the rows that are not -1
 *                    (GI_LL_ERR_ORDER); on a violation, and while err carries one of these two bits from an earlier
 *                    call, the launch writes nothing. */
#define GI_LL_ERR_HOT 1             /* a hot index outside [-1, W) */
#define GI_LL_ERR_MOL 2             /* a row_mol outside [-1, n_mol) */
#define GI_LL_ERR_ORDER 4           /* row_mol decreases */
int gi_row_loglik(const float* logits, long long ld, int rows, int W, const int* hot, float* row_ll, float* row_lse,
                  int* err, void* stream);
int gi_row_loglik_bwd(const float* logits, long long ld, int rows, int W, const int* hot, const float* row_lse,
                      const float* g_mol, const float* g_kind, const int* row_mol, int n_mol, int n_add, int n_conn,
                      float* d_logits, long long ldd, int* err, void* stream);
int gi_mol_loglik_sum(const float* row_ll, const int* row_mol, const int* hot, int rows, int n_mol, int W, int n_add,
                      int n_conn, float* mol_ll, float* mol_kind, int* err, void* stream);

/* Node reordering (gi_reorder.hip): what `PreprocessingGraph.node_remap` (MolecularGraph.py:435-461) does once it has
 * a node ranking, for M molecules in one launch: a breadth- or depth-first search (:328-433) from node rank[0], then
 * `reorder_nodes` and `pad_graph_representation` (:592-633).  nodes [M, N, Fn] / edges [M, N, N, Fe] as above, except
 * that the nodes may be in ANY order; out_nodes / out_edges (same shapes, not the inputs) hold nodes[order] and
 * edges[order][:, order], zero padded, which satisfy gi_route_plan's order rule.  No alignment or padding is asked of
 * any buffer.
 *
 * rank [M, N] int32 (device): the first n entries of a row are a permutation of 0 .. n-1, higher = more important
 * (the reference's `atom_ranking`); NULL draws it on the device from (seed, epoch, id), id = mol_ids[m] (int64,
 * device) or m when mol_ids is NULL: s = mix64(mix64(seed) + epoch), key_i = mix64(s ^ (id << 8 | i)) with the
 * splitmix64 step mix64 and 64-bit wrap-around, rank_i = the number of j < n with (key_j, j) < (key_i, i).
 *
 * GI_ROUTE_DFS is the reference's loop, node for node.  GI_ROUTE_BFS emits every level in ascending input index: the
 * level SETS are the reference's, whose order inside a level is CPython's set iteration order (equal to this one for
 * molecules of up to 8 nodes, not in general beyond).  The ranking reaches a BFS through the start node only.
 *
 * order [M, N] int32 (NULL: not written): the input index of every output node, -1 past the molecule's n nodes.
 * mol_err [M]: 0, or the GI_ROUTE_ERR_* bits of a molecule the kernel refuses — an entry not 0 / 1 (VALUE), nodes
 * not a zero-padded prefix or a bond on padding or the diagonal (PADDING), asymmetric edges, no node (EMPTY), not
 * connected (CONNECT), `rank` not a permutation (RANK).  Such a molecule is copied through unchanged, order = the
 * identity; every loop is bounded by the dims, nothing faults and nothing is written out of bounds. */
#define GI_ROUTE_ERR_RANK 128       /* a given rank row is not a permutation of 0 .. n-1 */
#define GI_ROUTE_BFS 0
#define GI_ROUTE_DFS 1
int gi_route_reorder(int M, int N, int Fn, int Fe, const signed char* nodes, const signed char* edges,
                     const int* rank, unsigned long long seed, unsigned long long epoch, const long long* mol_ids,
                     int mode, signed char* out_nodes, signed char* out_edges, int* order, int* mol_err,
                     void* stream);

/* Read-out of molecules (gi_analyze.hip): the tensor bookkeeping of `Analyzer.get_molecular_properties`
 * (Analyzer.py:311-599) and of `graph_to_graph` (GraphGenerator.py:659-804) for G graphs in one launch each.
 * nodes [G, N, Fn] / edges [G, N, N, Fe]: contiguous, GI_DTYPE_F32 or GI_DTYPE_I8, entries expected to be 0 / 1 (the
 * statistics take any integer of magnitude <= 128).  n_nodes [G]: integers of n_nodes_bytes = 1, 4 or 8 bytes.  No
 * alignment is asked of any input.  N <= GI_MAX_NODES and Fe <= GI_MAX_GROUPS (GI_EINVAL otherwise); Fn <=
 * GI_ANALYZE_MAX_FN (GI_ELIMIT).  G = 0 returns 0 without a launch and without touching any buffer.
 *
 * gi_mol_properties: with H = max_n_nodes + 1 (max_n_nodes <= GI_ANALYZE_MAX_HIST), out (fp32) =
 *   [ n_nodes_hist H | column sums of the node rows Fn | n_edges_hist GI_ANALYZE_EDGE_BINS | edge_feature_hist Fe |
 *     avg_n_nodes | avg_n_edges | fraction_properly_terminated ]
 * as the reference defines them: hist[n_nodes] += 1 (a count outside [0, min(N, max_n_nodes)] is not binned); the
 * column sums over ALL N rows; for every node < n_nodes the degree over all N columns and all bond types, clamped to
 * the bin count and counted at degree - 1, degree 0 in the LAST bin; per bond type the sum of the whole [N, N] plane
 * / 2; the averages sum(n count) / G and sum((bin + 1) count) / sum(count) (0 / 0 = NaN); sum(termination) / G
 * (termination [G] GI_DTYPE_I8 or GI_DTYPE_F32; NULL: 0).  n_nodes = NULL counts the non-zero node rows instead.
 * Counts are summed as integers (any order gives the same result) and converted once: the exact integer as fp32,
 * then one fp32 division, which is the reference's value bit for bit while every count is below 2^24.
 * totals: H + Fn + GI_ANALYZE_EDGE_BINS + Fe + 2 64-bit words, ZERO on entry; they hold the integer counts (then
 * the termination sum and a launch counter) on return.
 *
 * gi_mol_decode (n_nodes required): seg[n_seg] (HOST, 2 <= n_seg <= 4, entries 1 .. 127, sum Fn) are the one-hot
 * segments of a node row.  atoms [G, N, n_seg] int8: for a node < n_nodes the index inside each segment of its
 * first non-zero entry (-1: none), -1 for the other nodes.  bonds [G, max_bonds, 3] int16: the triples (i, j, type)
 * with i < j of the non-zero entries of the WHOLE [N, N, Fe] tensor, in row-major order of (i, j, type), padded
 * with -1; n_bonds [G] their true number.  status [G]: the GI_MOL_* bits. */
#define GI_ANALYZE_MAX_FN 512
#define GI_ANALYZE_MAX_HIST 1024
#define GI_ANALYZE_EDGE_BINS 10
#define GI_MOL_ONEHOT 1             /* a node row < n_nodes without exactly one non-zero entry in some segment */
#define GI_MOL_BOND_PAST_N 2        /* a bond touches a node >= n_nodes */
#define GI_MOL_OVERFLOW 4           /* more than max_bonds bonds: the first max_bonds are written */
#define GI_MOL_VALUE 8              /* an entry of nodes or edges is neither 0 nor 1 */
#define GI_MOL_MULTI_BOND 16        /* a pair i < j carries several bond types (every triple is emitted) */
int gi_mol_properties(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                      const void* n_nodes, int n_nodes_bytes, const void* termination, int term_dtype,
                      int max_n_nodes, unsigned long long* totals, float* out, void* stream);
int gi_mol_decode(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                  const void* n_nodes, int n_nodes_bytes, int n_seg, const int* seg, int max_bonds,
                  signed char* atoms, short* bonds, int* n_bonds, int* status, void* stream);

/* Molecule identity (gi_canon.hip): which molecules of a batch are the same labelled graph — node feature rows and
 * bond types, nothing else — which the reference decides on the host from canonical SMILES (util.py:549-585,
 * Analyzer.py:480-499).  nodes / edges / n_nodes / dtype as for gi_mol_decode; n_nodes = NULL takes the number of
 * LEADING node rows with a set entry.  The nodes may be in any order; bonds may carry several types and loops.
 *
 * gi_mol_canon, one launch: per molecule a canonical node order by colour refinement with individualisation.  With
 * mix64 the splitmix64 step of gi_route_reorder and all sums modulo 2^64:
 *   col_i  = #{j < n : row_j < row_i}, feature rows compared as byte strings;
 *   round:   h_i = sum over (t, j) with edges[i, j, t] set of mix64(t << 32 | col_j),
 *            col'_i = #{j : (col_j, h_j) < (col_i, h_i)}; rounds repeat until the number of distinct colours stops
 *            growing;
 *   while colours repeat: in the non-singleton cell of smallest colour r the member of lowest input index keeps r,
 *            the others get r + 1; rounds again.  There is NO backtracking: a molecule with a refinement cell that is
 *            not an automorphism orbit may get different orders from different input orders;
 *   order [G, N] int32 = the input index of every canonical position (-1 past n), rank [G, N] its inverse;
 *   out_nodes [G, N, Fn] / out_edges [G, N, N, Fe] int8 (either may be NULL; not the inputs) = nodes[order],
 *            edges[order][:, order], zero padded;
 *   key [G, 2] (64-bit words): k0 = mix64(n) + sum mix64(1 << 40 | a Fn + f) + sum mix64(2 << 40 | (a N + b) Fe + t)
 *            over the set entries (a, f) / (a, b, t) of the canonical molecule, k1 the same with the tags 3, 4, 5 in
 *            place of none, 1, 2; a word that comes out 0 is stored as 1.
 * status [G]: GI_MOL_VALUE, GI_MOL_BOND_PAST_N, GI_MOL_ASYMMETRIC (edges[i, j, t] set, edges[j, i, t] not),
 * GI_MOL_NODE_PAST_N (a node row >= n has a set entry, or n_nodes is outside [0, N]).  A molecule with a non-zero
 * status gets order = rank = the identity over all N slots, a zero canonical molecule and the key
 * (mix64(6 << 40 | g), mix64(7 << 40 | g)) of its index g; the two entry points below never find it equal to anything.
 * At most 2 N + 2 rounds run whatever the data holds.  Fn <= GI_ANALYZE_MAX_FN (GI_ELIMIT).
 *
 * gi_mol_unique: first occurrences inside one call.  mask [G] int8 (NULL: all ones) says which molecules take part.
 * Two molecules are the same if both have status 0, equal keys AND byte-identical canonical molecules.  rep [G] = the
 * lowest index of the molecule's class, -1 where mask is 0; unique [G] fp32 = 0 where mask is set and rep < the
 * molecule's index, 1 elsewhere (util.py:549-573: an invalid molecule keeps 1 and is not remembered); counts
 * [GI_MOL_COUNTS] (zeroed here) = the OR of all G status words, the masked-in molecules, the classes among them.  The
 * result does not depend on timing.  ws: gi_mol_unique_ws_bytes(G) bytes.
 *
 * gi_mol_seen_add: across calls, by the 128-bit KEY ALONE (the molecules are not kept).  table: `capacity` (a power
 * of two) pairs of 64-bit words, zero = empty, owned and zeroed once by the caller; info [2] int32, zeroed with it:
 * [0] the number of keys stored, [1] GI_SEEN_FULL once a key found every slot taken by others.  For a molecule with
 * rep[i] == i and status 0: is_new[i] = 1 and the key is stored if it was not in the table, else 0.  Other molecules
 * get 0, except that one with rep[i] == i and a non-zero status gets 1 and is not stored.  A probe visits at most
 * `capacity` slots and waits for nobody; when the table is full the key is not stored (is_new stays 1) and which keys
 * of that call were stored depends on timing. */
#define GI_MOL_ASYMMETRIC 32        /* gi_mol_canon: edges[i, j, t] is set and edges[j, i, t] is not */
#define GI_MOL_NODE_PAST_N 64       /* gi_mol_canon: a node row >= n has a set entry, or n_nodes outside [0, N] */
#define GI_MOL_COUNTS 3
#define GI_SEEN_FULL 1
int gi_mol_canon(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                 const void* n_nodes, int n_nodes_bytes, int* order, int* rank, unsigned long long* key,
                 int* status, signed char* out_nodes, signed char* out_edges, void* stream);
long long gi_mol_unique_ws_bytes(int G);
int gi_mol_unique(int G, int N, int Fn, int Fe, const unsigned long long* key, const signed char* canon_nodes,
                  const signed char* canon_edges, const int* status, const signed char* mask, void* ws, int* rep,
                  float* unique, int* counts, void* stream);
int gi_mol_seen_add(int G, const unsigned long long* key, const int* status, const int* rep,
                    unsigned long long* table, long long capacity, int* info, int* is_new, void* stream);

/* Molecule validity (gi_valence.hip): a valence test of the labelled graph and the hydrogen fill, the part of the
 * reference's validity_tensor (util.py:549-585, Analyzer.py:501-544; one SanitizeMol per molecule on the host) that the
 * tensors decide for the bond set single / double / triple.  NOT RDKit: no kekulisation and no aromaticity perception
 * is done, and the table of allowed valences is the caller's.  nodes / edges / n_nodes / dtype as for gi_mol_canon
 * (n_nodes = NULL: the number of LEADING node rows with a set entry).
 *
 * gi_mol_valence, one launch.  A node row is [ atom type n_types | formal charge n_charges | implicit H n_imp_h (may be
 * 0) | anything else (chirality; never looked at beyond "the row has a set entry") ], n_types + n_charges + n_imp_h <=
 * Fn.  Device tables: allowed [n_types * n_charges] (16 bits each: bit v set = total valence v is allowed for that
 * atom type and charge), mass [n_types] (int32, millidalton), order2 [Fe] (int8, twice the bond order), h_values
 * [n_imp_h] (int8, the hydrogen count every entry of the implicit-H segment stands for; NULL if n_imp_h = 0).  h_type:
 * the atom type that is hydrogen (-1: none), mass_h: its mass.  termination [G] (GI_DTYPE_I8 or _F32; NULL: nothing
 * is terminated).
 *
 * status [G]: a molecule with one of GI_MOL_VALUE, _NODE_PAST_N, _BOND_PAST_N, _ASYMMETRIC (as gi_mol_canon),
 * GI_MOL_ONEHOT (a row < n without exactly one non-zero entry in the type, charge or implicit-H segment) or
 * GI_MOL_MULTI_BOND (some pair i != j carries several bond types) is MALFORMED: it is invalid, atom_valence / atom_h
 * are -1 for all N slots, first_bad is -1, desc is zero and no GI_VAL_* bit other than _EMPTY and _SELF_LOOP is
 * evaluated.  Otherwise, per atom i < n, in integers:
 *   o2 = sum over t of order2[t] * #{j : edges[i, j, t]},  x = ceil(o2 / 2),
 *   v* = the smallest allowed valence >= x; none: the atom is OVER (fill 0); else the fill is h = v* - x.
 * atom_valence [G, N] int8 = min(x, 127), atom_h [G, N] int8 = the fill, both -1 at i >= n; first_bad [G] = the
 * lowest atom that is over, -1 if none; desc [G, GI_VAL_DESC] int32 = n_atoms, n_h (the fills plus the atoms of type
 * h_type), mass_mda (sum of mass[type] + fills * mass_h), n_bonds (pairs i < j with a bond), n_components, n_rings =
 * n_bonds - n_atoms + n_components.  valid [G] fp32 = 1 unless a GI_MOL_* bit above, GI_VAL_EMPTY, _SELF_LOOP or _OVER
 * is set (or _FRAGMENTS, with require_connected != 0).  counts [GI_VAL_COUNTS] int32: valid molecules, terminated
 * ones, valid and terminated ones, G; integer sums, so every output is deterministic.  scratch [GI_VAL_SCRATCH] int32:
 * owned by the caller, ZERO before its first use and left zero by every completed call (the workgroup that finishes
 * last moves the sums into counts and clears it, so nothing has to be cleared by a launch or a memset); calls that
 * share a scratch must be ordered, e.g. issued on one stream.  G = 0 returns 0 and touches nothing.  Every loop is
 * bounded by the dims whatever the data holds (components: at most N rounds). */
#define GI_VAL_EMPTY 128            /* n == 0 (the reference's mol = None ends at validity 0) */
#define GI_VAL_SELF_LOOP 256        /* edges[i, i, t] is set (AddBond refuses it) */
#define GI_VAL_OVER 512             /* some atom exceeds every allowed valence of its type and charge */
#define GI_VAL_FRAGMENTS 1024       /* more than one component (invalid only with require_connected) */
#define GI_VAL_AROMATIC 2048        /* a bond of order 1.5 is present: counted 3 per 2, no kekulisation (informational) */
#define GI_VAL_H_MISMATCH 4096      /* an atom's stored implicit-H count differs from its fill (informational) */
#define GI_VAL_DESC 6
#define GI_VAL_COUNTS 4
#define GI_VAL_SCRATCH 4
int gi_mol_valence(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                   const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                   const unsigned short* allowed, const int* mass, const signed char* order2,
                   const signed char* h_values, int h_type, int mass_h, const void* termination, int term_dtype,
                   int require_connected, float* valid, int* status, int* first_bad, signed char* atom_valence,
                   signed char* atom_h, int* desc, int* counts, int* scratch, void* stream);

/* Molecule scores (gi_fingerprint.hip): a packed circular fingerprint per molecule, and a batch of fingerprints against
 * a stored set — what the reference's "activity" score (ScoringFunction.py:145-192: one RDKit Morgan fingerprint and
 * one scikit-learn predict_proba per molecule, on the host) needs, plus nearest-neighbour similarity.  THE FINGERPRINT
 * IS A MORGAN-STYLE FINGERPRINT OF THE LABELLED GRAPH, NOT RDKit's ECFP BITS: other atom invariants (no ring
 * membership, no isotope, hydrogens only through the bond-order sum), another hash, no removal of duplicate
 * substructures, no aromaticity perception; a model must be trained on THESE fingerprints.  Guaranteed: isomorphic
 * labelled molecules get equal rows in any node order, and id_r is equal for two atoms exactly when their radius-r
 * labelled neighbourhoods are 1-WL-equivalent (up to 64-bit hash collisions).  tests/fingerprint_model.py is the numpy
 * specification (and holds the constants K0, K1).
 *
 * gi_mol_fingerprint, one launch, one workgroup per molecule.  nodes / edges / n_nodes / dtype and the node row's
 * segments n_types | n_charges | n_imp_h as for gi_mol_valence; order2 [Fe] (int8, device) twice the bond order.  A
 * molecule is read and checked exactly as gi_mol_valence does it: with any of GI_MOL_VALUE, _NODE_PAST_N, _BOND_PAST_N,
 * _ASYMMETRIC, _ONEHOT, _MULTI_BOND, GI_VAL_EMPTY (n == 0) or GI_VAL_SELF_LOOP its row is all zero, popcount 0, atom_id
 * -1, status [G] holds the bits, and nothing else is evaluated.  Otherwise status is 0 and, in 64-bit wrap-around
 * arithmetic with mix64 the splitmix64 finaliser, for the atoms i < n:
 *   id_0[i] = mix64(K0 + a_i + 256 c_i + 2^16 deg_i + 2^24 o2_i)    a_i / c_i: the index inside the atom-type / charge
 *             segment, deg_i: the bonded partners, o2_i = sum over t of order2[t] * #{j : edges[i, j, t]}; the
 *             implicit-H and chirality segments do not enter;
 *   id_r[i] = mix64(mix64(id_{r-1}[i] + r) + sum over the bonds (t, j) of i of mix64(id_{r-1}[j] ^ (K1 order2[t]))),
 *             r = 1 .. radius, 0 <= radius <= GI_FP_MAX_RADIUS (the sum is commutative: no order enters);
 *   bits [G, n_bits / 32] int32 (16-byte aligned): bit (id_r[i] & (n_bits - 1)) for every r <= radius and i < n; bit b
 *             is bit b & 31 of word b >> 5; n_bits a power of two in [GI_FP_MIN_BITS, GI_FP_MAX_BITS];
 *   popcount [G] int32 the set bits of the row; atom_id [G, N, 2] int32 (may be NULL): the low and the high half of
 *             id_radius[i], -1 for i >= n.
 * Integer arithmetic only: every output is deterministic.  No global atomics, no scratch; every loop is bounded by N,
 * Fe and radius.  radius or n_bits outside their limits: GI_EINVAL.  G = 0 returns 0 and touches nothing.
 *
 * gi_fp_compare, one launch: G query rows against S >= 1 set rows of W = n_bits / 32 words (query [G, W_query], set
 * [S, W_set], int32, both 16-byte aligned; W_query != W_set, a W that no n_bits gives, or S < 1: GI_EINVAL).  Per pair
 * c = popcount(q & s), a = popcount(q), b = popcount(s), u = a + b - c.  Always: the set row of the largest Tanimoto
 * c / u (0 / 0 := 0), decided in integers by cross-multiplication, ties to the lowest set index: nearest [G] (-1 where
 * a == 0), common [G] = its c, uni [G] = its u (both 0 where a == 0), max_sim [G] fp32 = (float)c / (float)u, one
 * correctly rounded division (0 where a == 0).  With weight [S] fp32 (else decision / proba may be NULL and are not
 * written): decision [G] fp32 = intercept + sum over s of weight[s] K(q, s), K = c / u (GI_FP_TANIMOTO; 0 where
 * u == 0), exp(-gamma (a + b - 2 c)) (GI_FP_RBF: the squared distance of 0 / 1 vectors) or c (GI_FP_LINEAR); proba
 * [G] fp32 = 1 / (1 + exp(prob_a decision + prob_b)), and 0 where a == 0 (an empty or malformed molecule scores
 * nothing: the reference's `except: pass`).  The fp32 sum is made in a FIXED order — each of 256 lanes adds its rows
 * s = l, l + 256, .. in ascending order, the 64 lanes of a wave meet in a 6-level xor butterfly, the four waves are
 * added in order, the intercept last; the longest chain of additions is ceil(S / 256) + 9 — so equal inputs give equal
 * bits on every run.  No atomics.  G = 0 returns 0 and touches nothing. */
#define GI_FP_MIN_BITS 64
#define GI_FP_MAX_BITS 4096
#define GI_FP_MAX_RADIUS 4
#define GI_FP_TANIMOTO 0
#define GI_FP_RBF 1
#define GI_FP_LINEAR 2
int gi_mol_fingerprint(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                       const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                       const signed char* order2, int radius, int n_bits, int* bits, int* popcount, int* status,
                       int* atom_id, void* stream);
int gi_fp_compare(int G, int S, int W_query, int W_set, const int* query, const int* set, const float* weight,
                  int kind, double gamma, double intercept, double prob_a, double prob_b, int* nearest, int* common,
                  int* uni, float* max_sim, float* decision, float* proba, void* stream);

/* Molecule strings (gi_smiles.hip): every molecule as a SMILES string, the product of the reference's
 * write_graphs_to_smi (util.py:520-585; one RWMol, one SanitizeMol and one MolToSmiles per molecule on the host).  THE
 * STRING IS A FAITHFUL SPELLING OF THE LABELLED GRAPH in an OpenSMILES subset, NOT RDKit's CANONICAL SMILES: no
 * aromaticity perception or kekulisation, no stereo marks (the reference sets no chiral tag either: graph_to_mol keeps
 * chirality only as the _CIPCode property), hydrogen counts from the caller's table or from the stored segment.
 * tests/smiles_model.py is the Python specification, with an independent reader.
 *
 * gi_mol_smiles, one launch, one workgroup per molecule, no global atomics, nothing to clear before it.  nodes / edges
 * / n_nodes / dtype, the node row's segments n_types | n_charges | n_imp_h, allowed and order2 as for gi_mol_valence.
 * charges [n_charges] (int8, device): the formal charge of every entry; symbols [n_types, 2] (bytes, device): the
 * element symbol, the second byte 0 for a one-letter symbol; h_values [n_imp_h] as for gi_mol_valence.  stored_h = 0:
 * an atom's hydrogen count h is the fill of gi_mol_valence (v* - x, 0 for an atom over its valence); stored_h = 1
 * (needs n_imp_h > 0): the count its implicit-H entry stands for.  rank [G, N] (int32, device; NULL: the input index):
 * the traversal key of atom i is its place in the order by (rank[i], i), so any values are accepted; gi_mol_canon's
 * rank makes the string canonical in gi_mol_canon's sense (its documented incompleteness included).
 *
 * The string.
 *   atom token   bare symbol when the symbol is one of B C N O P S F Cl Br I, the charge is 0 and h equals the OpenSMILES
 *                implicit count for the bond-order sum x = ceil(o2 / 2): v - x with v the smallest of the element's
 *                normal valences >= x (B 3, C 4, N 3 5, O 2, P 3 5, S 2 4 6, halogens 1), 0 without one.  Otherwise
 *                '[' symbol, 'H' if h >= 1, h if h >= 2, '+' or '-' and the magnitude if >= 2, ']'.  An atom of type
 *                "H" is always "[H]" with its charge, never a count.  A token has at most 12 bytes.
 *   bonds        a single bond is elided, a double bond is '=', a triple bond '#'.
 *   order        components in ascending order of their lowest-key atom, joined by '.'; each is walked depth-first from
 *                that atom, neighbours in ascending key: one that is unvisited when it is reached becomes a tree child,
 *                one that is visited and is not the tree parent is a ring bond.  Atoms appear in pre-order.
 *   at an atom   1 the token; 2 its ring closings in ascending pre-order index of the partner, each the bond symbol and
 *                the number, which is free again at once; 3 its ring openings in the same order, each the smallest free
 *                number >= 1 without a bond symbol; 4 its children in visiting order, every one but the last in
 *                parentheses, the bond symbol directly in front of the child's token, inside the parenthesis.
 *   numbers      1-9 one digit, 10-99 "%nn".  Kekule benzene in ring order is "C1=CC=CC=C1".
 *
 * text [G, max_len] bytes (16-byte aligned), zero padded; max_len a multiple of 16 in [16, GI_SMI_MAX_LEN] (beyond:
 * GI_ELIMIT; the limit keeps the string, the ring tokens and the adjacency rows of N = 128, Fe = 8 inside 64 KB of
 * LDS).  No bound short of N^2 bytes holds for every legal input — a clique of n atoms carries (n - 1)(n - 2) / 2 ring
 * bonds — so 12 N + 4 is a default, not a bound: it holds a molecule whose every atom has an 8-byte bracket token, a bond
 * symbol, a branch of its own and a ring digit.  length [G]: the bytes of the string.  atom_pos [G, N] int32: the byte offset of every
 * atom's token, -1 for i >= n and throughout a molecule with an empty text.  status [G]: the GI_MOL_* bits of a
 * malformed molecule exactly as gi_mol_valence sets them (GI_MOL_MULTI_BOND included) and the bits below, the first
 * five with the values and meanings of GI_VAL_EMPTY .. GI_VAL_AROMATIC.  A malformed molecule, GI_SMI_EMPTY,
 * _SELF_LOOP, _AROMATIC and _RING_LIMIT give an empty text, length 0 and atom_pos -1; GI_SMI_TRUNCATED gives an empty
 * text and atom_pos -1 with length = the bytes needed, so that the caller can ask again; GI_SMI_OVER and
 * GI_SMI_FRAGMENTS are informational, the string is written.  G = 0 returns 0 and touches nothing.  Every loop is
 * bounded by N, Fe, the 32 bits of a word or 2 N + 1 (the walk) whatever the data holds. */
#define GI_SMI_EMPTY 128            /* n == 0 */
#define GI_SMI_SELF_LOOP 256        /* edges[i, i, t] is set */
#define GI_SMI_OVER 512             /* some atom exceeds every allowed valence of its type and charge (informational) */
#define GI_SMI_FRAGMENTS 1024       /* more than one component: the string has a '.' (informational) */
#define GI_SMI_AROMATIC 2048        /* a bond of order 1.5 is present: nothing is kekulised, no string */
#define GI_SMI_RING_LIMIT 8192      /* more than 99 ring bonds are open at once */
#define GI_SMI_TRUNCATED 16384      /* the string needs more than max_len bytes; length holds the need */
#define GI_SMI_MAX_LEN 8192
int gi_mol_smiles(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                  const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                  const unsigned short* allowed, const signed char* order2, const signed char* h_values,
                  const signed char* charges, const unsigned char* symbols, int stored_h, const int* rank,
                  int max_len, unsigned char* text, int* length, int* status, int* atom_pos, void* stream);

/* Molecule reading (gi_smiles_read.hip): SMILES strings into molecules, the inverse of gi_mol_smiles ON THE WRITER'S
 * SUBSET of OpenSMILES — what the reference's preprocessing gets from one MolFromSmiles and one graph construction per
 * molecule on the host.  NOT RDKit: NO AROMATIC INPUT (nothing is kekulised) AND NO STEREO; such a string gets a status
 * bit and no molecule, so that the caller can route it to RDKit (gi_smiles_read_arom below reads aromatic input, and
 * kekulises it by a rule of its own).  Atoms are numbered IN STRING ORDER, which is not the
 * order of the reference's preprocessing.  tests/smiles_read_model.py is the Python specification, stage by stage.
 *
 * gi_smiles_read, one launch, one workgroup per string, integers only, no global atomics, no scratch, nothing to clear
 * before it.  text [G, max_len] bytes (16-byte aligned; gi_mol_smiles' own layout), max_len a multiple of 16 in
 * [16, GI_SMI_MAX_LEN] (beyond: GI_ELIMIT); length [G] int32, or NULL: the string ends at its first zero byte (at max_len
 * without one).  A length outside [0, max_len] is GI_SMR_SYNTAX.  The node row's segments n_types | n_charges | n_imp_h
 * and the device tables symbols [n_types, 2], charges [n_charges], h_values [n_imp_h], order2 [Fe] and allowed as for
 * gi_mol_smiles.  none_chirality: where n_types + n_charges + n_imp_h < Fn, the entry set inside the rest of every
 * atom's row (0 <= none_chirality < the rest, GI_EINVAL otherwise; the reference's chirality list puts 'None' first).
 * drop_stereo 0 or 1.
 *
 * The grammar: what gi_mol_smiles writes, plus what OpenSMILES lets other writers say about the same graphs.
 *   bracket atom '[' symbol, 'H' and a count, '+' or '-' and a magnitude ']': the symbol a capital and at most one small
 *                letter; 'H' alone counts 1, a sign alone 1; counts saturate at 1000.  "[H]" is an atom of type "H".
 *   bare atom    B C N O P S F Cl Br I (bare H is GI_SMR_SYNTAX).
 *   bonds        '-' '=' '#' in front of an atom or a ring number; none: a single bond.
 *   branches     '(' behind an atom, nested up to 128 deep; "((" and "()" are GI_SMR_SYNTAX.
 *   rings        a digit or "%nn" behind an atom opens a ring number or closes the open one; a bond symbol may stand on
 *                either end and must agree if it stands on both; a closed number may be used again.
 *   '.'          between components.
 * Hydrogens: a bare atom has the OpenSMILES implicit count for its bond-order sum x (v - x with v the smallest normal
 * valence >= x of B 3, C 4, N 3 5, O 2, P 3 5, S 2 4 6, halogens 1; 0 without one: the table gi_mol_smiles calls an atom
 * bare by), a bracket atom the count it states.  With n_imp_h > 0 the count is stored as its entry of the implicit-H
 * segment; with n_imp_h = 0 nothing is stored.
 *
 * nodes [G, N, Fn] / edges [G, N, N, Fe] int8 (any alignment; edges symmetric, one-hot per bonded pair), n_nodes [G],
 * status [G], atom_pos [G, N] int32 (the byte offset of every atom's token, -1 for i >= n: gi_mol_smiles' output).
 * Every byte of every output is written, the node and edge rows in 16-byte stores between the ragged ends of their
 * address range.  A string with any bit of GI_SMR_ERROR gives the all-zero molecule — what the rest of the library
 * treats as empty — with n_nodes 0 and atom_pos -1; GI_SMR_TOO_MANY alone keeps n_nodes = the atoms the string needs,
 * so that the caller can ask again.  The bits are set in stages (bytes; atom tokens; the walk over the other tokens,
 * which ends at its first error; hydrogens) and a stage runs only while no error bit is set, GI_SMR_TOO_MANY skipping
 * all but the first: tests/smiles_read_model.py has the order.  Limits N <= GI_MAX_NODES, Fe <= GI_MAX_GROUPS (GI_EINVAL),
 * Fn <= GI_ANALYZE_MAX_FN (GI_ELIMIT).  G = 0 returns 0 and touches nothing.  Every loop is bounded by max_len, N, Fe,
 * the table widths or the 64 bits of a word whatever the bytes hold. */
#define GI_SMR_MULTI_BOND 16        /* the same pair bonded twice ("C12CC12"): GI_MOL_MULTI_BOND */
#define GI_SMR_EMPTY 128            /* the string is empty: GI_SMI_EMPTY */
#define GI_SMR_SELF_LOOP 256        /* a ring closes on the atom that opened it ("C11"): GI_SMI_SELF_LOOP */
#define GI_SMR_OVER 512             /* some atom exceeds every allowed valence of its type and charge (informational) */
#define GI_SMR_FRAGMENTS 1024       /* more than one component (informational) */
#define GI_SMR_AROMATIC 2048        /* a lowercase atom or ':': nothing is kekulised, no molecule */
#define GI_SMR_TOO_MANY 16384       /* more than N atoms; n_nodes holds the need (as GI_SMI_TRUNCATED's length does) */
#define GI_SMR_SYNTAX 65536         /* an unclosed bracket or branch, a dangling bond, a bond or ring digit without an atom
                                       to its left, "..", an unknown byte, '%' without two digits, bare H, a bad length */
#define GI_SMR_RING_OPEN 131072     /* a ring number is still open at the end */
#define GI_SMR_RING_ORDER 262144    /* the two ends of a ring bond state different orders */
#define GI_SMR_ELEMENT 524288       /* a symbol that is not in symbols */
#define GI_SMR_CHARGE 1048576       /* a charge that is not in charges */
#define GI_SMR_HCOUNT 2097152       /* a hydrogen count that is not in h_values (n_imp_h > 0 only) */
#define GI_SMR_BOND_ORDER 4194304   /* a bond order that is not in order2 */
#define GI_SMR_STEREO 8388608       /* '@' '/' '\' with drop_stereo = 0 */
#define GI_SMR_STEREO_DROPPED 16777216 /* the same with drop_stereo = 1: skipped, '/' '\' are single bonds (informational) */
#define GI_SMR_UNSUPPORTED 33554432 /* an isotope, an atom class, "++" / "--", '$', the wildcard */
#define GI_SMR_KEKULE 67108864      /* gi_smiles_read_arom, aromatic = 1: no Kekule structure (no perfect matching) */
#define GI_SMR_KEKULIZED 134217728  /* the same: the string had an aromatic atom and was read (informational) */
#define GI_SMR_ERROR (GI_SMR_MULTI_BOND | GI_SMR_EMPTY | GI_SMR_SELF_LOOP | GI_SMR_AROMATIC | GI_SMR_TOO_MANY | \
                      GI_SMR_SYNTAX | GI_SMR_RING_OPEN | GI_SMR_RING_ORDER | GI_SMR_ELEMENT | GI_SMR_CHARGE | \
                      GI_SMR_HCOUNT | GI_SMR_BOND_ORDER | GI_SMR_STEREO | GI_SMR_UNSUPPORTED | GI_SMR_KEKULE)
int gi_smiles_read(int G, int N, int Fn, int Fe, const unsigned char* text, const int* length, int max_len,
                   int n_types, int n_charges, int n_imp_h, const unsigned short* allowed, const signed char* order2,
                   const signed char* h_values, const signed char* charges, const unsigned char* symbols,
                   int none_chirality, int drop_stereo, signed char* nodes, signed char* edges, int* n_nodes,
                   int* status, int* atom_pos, void* stream);

/* gi_smiles_read with AROMATIC INPUT: the same arguments and `aromatic`, 0 or 1 (anything else: GI_EINVAL).  0 is
 * gi_smiles_read, the same kernel instantiation, byte for byte.  1 reads aromatic atoms and ':' and KEKULISES inside the
 * same launch: single and double bonds are assigned to the aromatic-marked bonds, since the library stores Kekule graphs
 * (the reference's use_aromatic_bonds False).  THE RULE IS OURS, NOT RDKit'S KEKULISATION: no ring or aromaticity
 * perception, no canonical choice among several Kekule structures; two strings of one compound can come out as two
 * different Kekule structures.  tests/kekule_read_model.py is the Python specification, in every output byte.
 *
 * Grammar added with aromatic = 1 (everything else as above; GI_SMR_AROMATIC is never set):
 *   bare atom    b c n o p s are aromatic atoms.  Any other small letter where a symbol is expected is GI_SMR_SYNTAX.
 *   bracket atom the symbol may be b c n o p s se as (OpenSMILES' list; another small symbol is GI_SMR_SYNTAX); it is
 *                looked up in symbols CAPITALISED; H count and charge as above ("[nH]", "[n+]", "[cH-]", "[se]").
 *   bonds        ':' is a bond symbol.  A bond with no symbol (a chain bond, or a ring bond with no symbol on either
 *                end) between two aromatic atoms is AROMATIC-MARKED, and so is ':'; ':' next to an atom that is not
 *                aromatic is GI_SMR_UNSUPPORTED; ':' on one end of a ring bond and another symbol on the other is
 *                GI_SMR_RING_ORDER.  '-' '=' '#' between aromatic atoms mean what they say.
 * Which atoms need a double bond: with sigma the atom's bond-order sum, every aromatic-marked bond counted 1, a bare
 * aromatic atom needs one when sigma is not a normal valence of its element (the table above) and a larger one exists;
 * a bracket aromatic atom when sigma + its stated H is not in allowed[type, charge] and a larger allowed valence exists.
 * So c needs one unless it has an exocyclic "=O", pyridine n needs one; three-coordinate n, [nH], o, s, [se], [n-] do
 * not; [n+], [o+], [s+] with two ring bonds and n(=O) do.  No other atom needs one.
 * The assignment: a perfect matching of the needing atoms over the aromatic-marked bonds between two needing atoms.
 * Matched bonds become the double type (order2 == 4), every other aromatic-marked bond the single type (order2 == 2); a
 * type that is needed and missing is GI_SMR_BOND_ORDER.  No perfect matching: GI_SMR_KEKULE and the all-zero molecule.
 * Which matching: a greedy pass over the atoms in ascending index, each matched to its lowest-index free candidate
 * neighbour, then one breadth-first augmenting-path search with blossom contraction (base / parent / queue) per needing
 * atom still free, in ascending index, neighbours scanned in ascending index.  An aromatic-marked bond between two
 * rings ("c1ccccc1c1ccccc1") is in every perfect matching or in none, by the parity of the needing atoms on its two
 * sides: biphenyl gets a single linker, "c1cccc1c1cccc1" is read as fulvalene.
 * Hydrogens are counted after the assignment, on the Kekule bonds, a bare aromatic symbol capitalised first.  The stage
 * runs after the walk and before the hydrogens, only while no error bit is set.  GI_SMR_KEKULIZED: the string had an
 * aromatic atom and no error bit. */
int gi_smiles_read_arom(int G, int N, int Fn, int Fe, const unsigned char* text, const int* length, int max_len,
                        int n_types, int n_charges, int n_imp_h, const unsigned short* allowed,
                        const signed char* order2, const signed char* h_values, const signed char* charges,
                        const unsigned char* symbols, int none_chirality, int drop_stereo, int aromatic,
                        signed char* nodes, signed char* edges, int* n_nodes, int* status, int* atom_pos, void* stream);

/* Constrained generation: the action mask between the forward and the draw of a generation round, in ONE launch with
 * no read-back (recordable into a hipGraph).  For each of B graphs (nodes [B, N, Fn] / edges [B, N, N, Fe], GI_DTYPE;
 * n_nodes [B], an entry of n_nodes_bytes = 1, 4 or 8 bytes, required) a COPY of its logits row is written in which
 * every inadmissible action is -inf and every other column keeps the input's bits:
 *   masked[b, j] = admissible(b, j) ? logits[b, j] : -inf,   j < W = N A + N Fe + 1,  A = prod(group) * Fe
 * (row pitches ldl / ldm >= W), and the same for an optional second matrix logits2 -> masked2 (the prior of RL
 * fine-tuning; its own pitches; both NULL: skipped).  gi_sample_actions / gi_sample_actions_rl, unchanged, then draw
 * from the renormalised distribution: their likelihoods are those of the CONSTRAINED policy.  A masked copy must not
 * be the matrix it is made from (GI_EINVAL): a model's backward reads its output.
 * THE VALENCE TABLE IS THE CALLER'S (allowed, order2, h_values as at gi_mol_valence), NOT RDKit'S SANITISATION.
 *
 * Columns, as gi_sample_actions decodes them: add(i, rem) at i A + rem, rem ravelled over (group[0], ..., group[n_groups
 * - 1], Fe) — the node-feature groups in node-row order (group[0] = n_types, group[1] = n_charges, group[2] = n_imp_h if
 * n_imp_h > 0, then whatever follows, e.g. chirality; sum = Fn), the bond type f last, as gi_grow_graphs unravels it;
 * connect(i, f) at N A + i Fe + f; terminate at W - 1.  n = n_nodes[b] clamped to [0, N].
 *
 * The state is WELL-FORMED when the labelled read (gi_mol_valence's) sets none of GI_MOL_ONEHOT, _BOND_PAST_N, _VALUE,
 * _MULTI_BOND, _ASYMMETRIC, _NODE_PAST_N and no GI_VAL_SELF_LOOP.  For such a state and an atom i < n, in integers:
 *   budget2(i) = 2 vmax(type_i, charge_i) - o2_i - 2 s_i
 * o2_i = sum_t order2[t] * #{j : edges[i, j, t]}, vmax the largest allowed valence (none allowed: -1), s_i the stored
 * hydrogen count h_values[.] (n_imp_h == 0: 0).
 * Structural rules, always applied:
 *   add(i, ...)    n < N, and i == 0 if n == 0, else i < n
 *   connect(i, f)  n >= 2, i < n - 1, no set entry in edges[b, i, n - 1, :]
 *   terminate      n >= 1, or allow_empty
 * Valence rules, for a well-formed state and valence = 1:
 *   add(i, type, charge, [h], ..., f), n >= 1   order2[f] <= budget2(i)  and  order2[f] + 2 h <= 2 vmax(type, charge)
 *   add, n == 0                                 2 h <= 2 vmax(type, charge), any f (the growth step sets no bond)
 *   connect(i, f)                               order2[f] <= budget2(i)  and  order2[f] <= budget2(n - 1)
 * A state that is not well-formed (the reference's dummy graph 0 always) gets the structural rules only.
 * With valid seeds this keeps flags & 1 of the sampler clear and every atom at or below its largest valence.
 *
 * Outputs: n_admissible [B]; status [B] = the malformed / self-loop bits above, plus GI_MASK_STRUCTURAL when any is set;
 * bits (optional) [B, ceil(W / 32)], column j = bit j & 31 of word j >> 5, zero past W; removed (optional) [B] fp32 =
 * the softmax mass of logits[b] (the first matrix) on the inadmissible columns (the only output not decided in
 * integers; 0 for a row without positive mass).  16-byte accesses where base and pitch allow, element-wise otherwise.
 * Limits: N <= GI_MAX_NODES, Fe <= GI_MAX_GROUPS, n_groups <= GI_GROW_MAX_GROUPS (GI_EINVAL); Fn <= GI_ANALYZE_MAX_FN,
 * n_types * n_charges * max(n_imp_h, 1) <= GI_MASK_MAX_COMBOS, W < 2^31 - 1024 (GI_ELIMIT); no limit on W of its own
 * beyond that (the sampler keeps its row limit).  `group` is a host array.  B = 0 returns 0 and touches nothing.  No
 * global atomics, no scratch, no memset; every loop is bounded by N, Fn, Fe, W.
 * tests/action_mask_model.py is the Python specification. */
#define GI_MASK_STRUCTURAL (1 << 20)    /* the state is not well-formed: structural rules only */
#define GI_MASK_MAX_COMBOS 4096
int gi_action_mask(int B, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                   const void* n_nodes, int n_nodes_bytes, int n_groups, const int* group, int n_types,
                   int n_charges, int n_imp_h, const unsigned short* allowed, const signed char* order2,
                   const signed char* h_values, int valence, int allow_empty, const float* logits, int ldl,
                   float* masked, int ldm, const float* logits2, int ldl2, float* masked2, int ldm2,
                   int* n_admissible, int* status, unsigned* bits, float* removed, void* stream);

/* Running figures of a constrained generation loop, one small launch, nothing read back: unless grow_state (the growth
 * step's state words, optional) shows a frozen round (state[0] >= state[2] or state[3] != 0),
 *   acc_counts[0] += 1,  acc_counts[1] += #{b : removed[b] > 0},  acc_mass[0] += sum_b removed[b]
 * in a fixed order of additions.  Calls on one accumulator must be ordered (one stream).  B = 0 returns 0. */
int gi_action_mask_stats(int B, const float* removed, const int* grow_state, int* acc_counts, float* acc_mass,
                         void* stream);

/* ---- substructure search (gi_substructure.hip) ------------------------------------------------------------------
 * Which of G molecules (inputs as gi_mol_valence: fp32 or int8, any alignment, n_nodes given or NULL: derived) contain
 * which of P PATTERNS, in one launch with no read-back: the host's one HasSubstructMatch per molecule and pattern.
 * THIS IS NOT SMARTS AND NOT RDKit'S MATCHER: no ring or recursive predicates, NO AROMATICITY PERCEPTION (a Kekule pattern
 * of a ring system matches the molecule's stored Kekule phase only; ask for "any bond type" on the ring bonds instead).
 *
 * A pattern is a connected labelled graph of 1 <= Np <= GI_SUB_MAX_ATOMS atoms.  Per atom: a set of atom types and a set
 * of formal charges (bit masks over the type / charge segment), `degree` (the exact number of bonded partners, -1: any)
 * and `min_h` (at least this many hydrogens by the fill of gi_mol_valence, which is 0 for an atom over its valence; -1:
 * any).  Per bond: a non-empty set of bond types (an Fe-bit mask).  A MATCH is an injective map of the pattern's atoms
 * to atoms < n under which every atom predicate holds and every pattern bond lands on a bond whose type is in its mask
 * (a monomorphism: the molecule may have further bonds).  A molecule with a bit of the labelled read (GI_MOL_ONEHOT,
 * _BOND_PAST_N, _VALUE, _MULTI_BOND, _ASYMMETRIC, _NODE_PAST_N, empty = 128, self-loop = 256) matches nothing.
 *
 * The PLAN of a pattern is part of the contract (the step counts depend on it): its atoms in breadth-first order from atom
 * 0, neighbours in ascending index; position k > 0 has a parent position (where it was discovered from) and its other
 * bonds to earlier positions, the back bonds, in ascending position.
 * The SEARCH runs per (molecule, pattern, anchor); the anchor is the atom tried as the image of position 0 (placing it
 * is not a step).  Depth first: at position k the candidates are
 *   compat[k] & (OR over the parent bond's mask of the adjacency rows of the parent's image) & ~used
 * in ascending atom index (after a backtrack: those above the image just abandoned).  Taking a candidate is one STEP;
 * its back bonds are then checked and a candidate that fails them is abandoned.  The search stops at the first full
 * assignment.  An anchor about to take a step after max_steps steps is given up: no match, counted in n_limited.
 * 1 <= max_steps <= GI_SUB_MAX_STEPS.
 *
 * The patterns travel as ONE int32 table, once on the host (patterns_host, checked on every call: header against the
 * dims, Np in range, the plan a permutation, parents earlier than their children, back bonds earlier and not the parent,
 * masks non-empty and inside their segment) and once on the device (patterns, 16-byte aligned, read by the kernel):
 *   [0, 8)        P, Np_max, n_types, n_charges, Fe, TW = ceil(n_types / 32), CW = ceil(n_charges / 32), B (a multiple of 4)
 *   record p      at 8 + p S, S = 4 + Np_max R + B, R = 8 + 4 ceil((TW + CW) / 4):  Np, 0, 0, 0, the rows, the back bonds
 *   row k         at 4 + k R of the record: parent position, parent bond mask, first back bond, number of back bonds,
 *                 pattern atom, degree, min_h, 0, TW words of type bits, CW words of charge bits ("any" = all bits set)
 *   back bond     at 4 + Np_max R + i of the record: position | mask << 8
 * Outputs, with Pout = P, or 1 with pattern_index [G] int32 (molecule g against pattern pattern_index[g] only; an index
 * outside [0, P) matches nothing and sets GI_SUB_PATTERN_INDEX):
 *   match [G, Pout] 0 / 1;  n_anchors [G, Pout] the atoms that are the image of pattern atom 0 in some match (the
 *   functional-group count when atom 0 is the group's centre);  anchors [G, Pout, 4] the same as a 128-bit mask;
 *   first [G, Pout, Np_max] the images of the pattern's atoms, in the pattern's own atom order, of the assignment found
 *   from the LOWEST matching anchor (-1 where none and past Np);  n_limited [G, Pout];  status [G] = the labelled-read
 *   bits, GI_SUB_STEP_LIMIT if any of its pairs had a limited anchor, GI_SUB_PATTERN_INDEX.
 * Limits: N <= GI_MAX_NODES, Fe <= GI_MAX_GROUPS (GI_EINVAL), Fn <= GI_ANALYZE_MAX_FN, Np_max <= GI_SUB_MAX_ATOMS, P <=
 * GI_SUB_MAX_PATTERNS, max_steps <= GI_SUB_MAX_STEPS (GI_ELIMIT).  G = 0 returns 0 and touches nothing.  Integers only,
 * no global atomics, no scratch, no memset; every loop is bounded by N, Np, Fe, P or max_steps.
 * tests/substructure_model.py is the Python specification. */
#define GI_SUB_MAX_ATOMS 32
#define GI_SUB_MAX_PATTERNS 65536
#define GI_SUB_MAX_STEPS (1 << 20)
#define GI_SUB_STEP_LIMIT (1 << 21)     /* an anchor of this molecule was given up at max_steps */
#define GI_SUB_PATTERN_INDEX (1 << 22)  /* pattern_index[g] is outside [0, P) */
int gi_mol_substructure(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                        const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                        const unsigned short* allowed, const signed char* order2, const int* patterns_host,
                        const int* patterns, long long pattern_words, const int* pattern_index, int max_steps,
                        int* match, int* n_anchors, int* anchors, int* first, int* n_limited, int* status,
                        void* stream);

/* ---- the resonance normal form: one identity per compound (csrc/gi_resonance.hip) ----
 * gi_mol_canon compares labelled graphs, so two Kekule structures of one compound are two molecules.  gi_mol_resonance
 * says which bonds change order between the Kekule structures of a molecule and writes the molecule with those bonds
 * moved to a channel of their own; on that NORMAL FORM gi_mol_canon / gi_mol_unique / gi_mol_seen_add see one compound.
 * THIS IS NOT AROMATICITY PERCEPTION (and not RDKit's): no Hueckel count, no chemistry table, no moving charges, no
 * tautomers.  Cyclobutadiene, cyclooctatetraene and pentalene are delocalised; pyrrole, furan, quinone and the five-ring
 * of indole are not: they have ONE Kekule structure, so identity needs nothing there.
 *
 * The rule, for a well-formed molecule (the labelled read of gi_mol_valence: any GI_MOL_* bit, GI_RES_EMPTY or
 * GI_RES_SELF_LOOP and nothing is delocalised), orders from order2 [Fe] (twice the bond order):
 *   d(i) = the number of order-2 bonds at atom i;  t(i) = the number of bonds of order 3 or 1.5 at atom i;
 *   V' = the atoms with d = 1 and t = 0 whose double-bond partner also has d = 1 and t = 0;
 *   G' = (V', the bonds of order 1 or 2 between two members of V'); the double bonds inside V' are a perfect matching
 *        M of G';
 *   a bond e = (a, b) of G' is DELOCALISED iff   order 2: G' - e (the edge removed) has a perfect matching;
 *                                                order 1: G' - a - b (both atoms removed) has a perfect matching;
 *   equivalently iff e lies on an M-alternating cycle.  No other bond is delocalised.
 *   Normal form: nodes unchanged; edges_out [G, N, N, Fe + 1] int8: a delocalised bond has channel Fe set and no other,
 *   every other set entry is as stored (1; 2 throughout a molecule with GI_MOL_VALUE, so that gi_mol_canon reports on
 *   the normal form what it reports on the stored molecule).
 * What follows, and tests/test_resonance_cpu.py checks:
 *   PHASE INVARIANCE  V' and G' do not depend on the stored phase and the verdict is a property of G': all Kekule
 *     structures of one compound (same atoms, charges and hydrogens, the double bonds another perfect matching of G')
 *     have the same normal form, byte for byte.  CONVERSE: equal normal forms mean the two stored structures are
 *     perfect matchings of one G'.
 *   ONLY RING BONDS  no acyclic bond is delocalised (butadiene has none).
 *   VALENCE-NEUTRAL  every atom's bond-order sum is unchanged by the normal form and by gi_mol_kekulize.
 *   A stored bond of order 1.5 is left as it is, keeps its atoms out of V' and raises GI_RES_AROMATIC (informational).
 * The verdict is definitional; HOW it is found is free.  Here: with M in hand, G' - e has a perfect matching iff one
 * augmenting path joins a and b, G' - a - b iff one joins the partners of a and b (breadth-first search with blossom
 * contraction, csrc/gi_res_search.h, 64 searches of a molecule at once); a path found closes an alternating cycle, all
 * of whose bonds are marked at once.
 * Outputs: status [G] (the labelled-read bits, GI_RES_AROMATIC), n_delocalized [G] (bonds), n_atoms [G] (atoms on
 * one), n_systems [G] (connected components of the delocalised bonds), delocalized [G, N, 4] (128-bit rows: bit j & 31
 * of word j >> 5 of row i = bond i-j is delocalised; the layout of gi_mol_substructure's anchors), edges_out as above or
 * NULL (then nothing is written and Fe may be GI_MAX_GROUPS; with edges_out, Fe + 1 > GI_MAX_GROUPS is GI_ELIMIT).
 *
 * gi_mol_kekulize is the inverse: edges [G, N, N, Fe + 1] (fp32 or int8), order2 [Fe].  An atom NEEDS a double bond
 * when it carries a channel-Fe bond; the candidate graph is the channel-Fe bonds; a perfect matching is looked for as
 * in gi_smiles_read_arom (greedy in ascending index, then one search per free atom, neighbours ascending; ONE lane).
 * Matched bonds get the first type of order 2, every other channel-Fe bond the first type of order 1; edges_out
 * [G, N, N, Fe] int8.  No perfect matching: GI_RES_NO_KEKULE; channel-Fe bonds and no type of order 1 or none of order
 * 2: GI_RES_BOND_ORDER; either, or an unsound molecule: all-zero edges.  The choice is a function of the indexed graph:
 * applied to canonical molecules (gi_mol_canon of the normal form) it is a canonical Kekule structure.
 * Both: G = 0 returns 0 and touches nothing.  Integers only, no global atomics, no scratch, no memset; every loop is
 * bounded by N or by the number of G' bonds.  tests/resonance_model.py is the Python specification. */
#define GI_RES_EMPTY 128                /* = GI_VAL_EMPTY */
#define GI_RES_SELF_LOOP 256            /* = GI_VAL_SELF_LOOP */
#define GI_RES_AROMATIC 2048            /* = GI_VAL_AROMATIC: a stored bond of order 1.5 (informational) */
#define GI_RES_BOND_ORDER (1 << 22)     /* gi_mol_kekulize: the rules lack a type of order 1 or of order 2 */
#define GI_RES_NO_KEKULE (1 << 26)      /* gi_mol_kekulize: the channel-Fe bonds have no perfect matching */
int gi_mol_resonance(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                     const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                     const signed char* order2, int* status, int* n_delocalized, int* n_atoms, int* n_systems,
                     int* delocalized, signed char* edges_out, void* stream);
int gi_mol_kekulize(int G, int N, int Fn, int Fe, const void* nodes, const void* edges, int dtype,
                    const void* n_nodes, int n_nodes_bytes, int n_types, int n_charges, int n_imp_h,
                    const signed char* order2, int* status, signed char* edges_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
