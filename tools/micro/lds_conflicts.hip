// Where the rollout kernel's LDS bank conflicts come from: one kernel per access pattern of mvi_core.hpp (same lane -> address maps, same
// instruction widths), each a loop of that one LDS instruction, to be run under
//   rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_LDS_ADDR_CONFLICT -- tools/micro/bin/lds_conflicts
// (tools/gpu_lds_conflicts.sh divides the counters by the instruction counts: conflict cycles per wave instruction of each pattern).
#include <hip/hip_runtime.h>

#include <cstdio>

constexpr int REPS = 4096;
typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double *lds0() {
    extern __shared__ double dyn[];
    return dyn;
}
#define SINK(v) asm volatile("" ::"v"(v))

// ---- stores ----
template <int STRIDE>   // doubles between lanes
__global__ void w_b64(double *out) {
    double *S = lds0();
    const int l = threadIdx.x;
    double v = l;
    for (int r = 0; r < REPS; r++) { S[(l * STRIDE + (r & 3)) % 2400] = v; asm volatile("" ::: "memory"); }
    if (out) out[l] = S[l];
}
template <int STRIDE>
__global__ void w_b128(double *out) {
    d2 *S = (d2 *)lds0();
    const int l = threadIdx.x;
    d2 v = {(double)l, 1.0};
    for (int r = 0; r < REPS; r++) { S[((l * STRIDE) / 2 + (r & 1)) % 1200] = v; asm volatile("" ::: "memory"); }
    if (out) out[l] = lds0()[l];
}
// ---- loads ----
template <int STRIDE>
__global__ void r_b64(double *out) {
    double *S = lds0();
    const int l = threadIdx.x;
    double acc = 0;
    for (int r = 0; r < REPS; r++) { double v = *(volatile double *)&S[(l * STRIDE + (r & 3)) % 2400]; SINK(v); }
    if (out) out[l] = acc;
}
template <int STRIDE>
__global__ void r_b128(double *out) {
    d2 *S = (d2 *)lds0();
    const int l = threadIdx.x;
    for (int r = 0; r < REPS; r++) { d2 v = *(volatile d2 *)&S[((l * STRIDE) / 2 + (r & 1)) % 1200]; SINK(v.x); SINK(v.y); }
    if (out) out[l] = 0;
}
template <int STRIDE>   // two adjacent doubles as ds_read2_b64
__global__ void r_2b64(double *out) {
    double *S = lds0();
    const int l = threadIdx.x;
    for (int r = 0; r < REPS; r++) {
        d2 ab;
        const unsigned addr = (unsigned)(((l * STRIDE + 2 * (r & 1)) % 2400) * 8);
        asm volatile("ds_read2_b64 %0, %1 offset1:1\n\ts_waitcnt lgkmcnt(0)" : "=v"(ab) : "v"(addr) : "memory");
        SINK(ab.x);
    }
    if (out) out[l] = 0;
}
// ---- the quad-lane sweep's stores: lane (instance q, row r, column c) -> joint base + 4 r + c, instances of the puppet's two passes ----
__global__ void w_quad(double *out, int pass) {
    double *S = lds0();
    const int l = threadIdx.x;
    const int q = l < 60 ? l / 12 : 4, rc = l < 60 ? l % 12 : 0;
    // first joints (x 12 doubles) of the instances: round 0 pass 0 = torso mid, torso q2, hooks 1-3 (q2 set at +408 doubles behind 528 of J);
    // round 1 pass 0 = limb 1 mid / q2, limb 2 mid / q2, limb 3 mid
    const int base0[5] = {0, 1056, 1056 + 72, 1056 + 96, 1056 + 120}, base1[5] = {216, 1056 + 216, 264, 1056 + 264, 312};
    const int b = pass ? base1[q] : base0[q];
    for (int r = 0; r < REPS; r++) { S[(b + 12 * (r & 3) + rc) % 2400] = (double)l; asm volatile("" ::: "memory"); }
    if (out) out[l] = S[l];
}
// ---- gathers of the pair phase: lane -> 12 * a (twists) / 15 * b (per-config vectors), the puppet's first 64 config pairs ----
__global__ void r_gather(double *out, const int *idx, int stride, int vec) {
    double *S = lds0();
    const int l = threadIdx.x, a = idx[l];
    for (int r = 0; r < REPS; r++) {
        if (vec) { d2 v = *(volatile d2 *)&S[(stride * a + 2 * (r & 1)) % 2400]; SINK(v.x); }
        else { double v = *(volatile double *)&S[(stride * a + (r & 3)) % 2400]; SINK(v); }
    }
    if (out) out[l] = 0;
}

// ---- the puppet's own lane -> address maps (pose records, composite records): one LDS instruction per pattern at the addresses the
//      lanes of the rollout kernel use, a lane without a role switched off (addr < 0).  Addresses in doubles from the slice's base. ----
__global__ void w_map64(double *out, const int *addr) {
    const int l = threadIdx.x, a = addr[l];
    const unsigned b = (unsigned)(a < 0 ? 0 : a) * 8u;
    const double v = l;
    if (a >= 0) for (int r = 0; r < REPS; r++) asm volatile("ds_write_b64 %0, %1" ::"v"(b), "v"(v) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (out) out[l] = lds0()[l];
}
__global__ void r_map64(double *out, const int *addr) {
    const int l = threadIdx.x, a = addr[l];
    const unsigned b = (unsigned)(a < 0 ? 0 : a) * 8u;
    if (a >= 0) for (int r = 0; r < REPS; r++) { double v; asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(b) : "memory"); SINK(v); }
    if (out) out[l] = lds0()[l];
}
__global__ void r_map128(double *out, const int *addr) {
    const int l = threadIdx.x, a = addr[l];
    const unsigned b = (unsigned)(a < 0 ? 0 : a) * 8u;
    if (a >= 0) for (int r = 0; r < REPS; r++) { d2 v; asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(b) : "memory"); SINK(v.x); }
    if (out) out[l] = lds0()[l];
}
template <int OFF1>     // the second double OFF1 doubles behind the first (rows 0 and 1 of a pose column: 4 in the 12-double record, 2 in a half-record)
__global__ void r_map2x64(double *out, const int *addr) {
    const int l = threadIdx.x, a = addr[l];
    const unsigned b = (unsigned)(a < 0 ? 0 : a) * 8u;
    if (a >= 0) for (int r = 0; r < REPS; r++) {
        d2 v;
        if (OFF1 == 4) asm volatile("ds_read2_b64 %0, %1 offset1:4\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(b) : "memory");
        else asm volatile("ds_read2_b64 %0, %1 offset1:2\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(b) : "memory");
        SINK(v.x);
    }
    if (out) out[l] = lds0()[l];
}

// The puppet's schedule (specialize.header(systems.puppet())): 34 joints, 22 dynamic configs, 10 bodies, G at 1696, G2 at 704, composites at 176.
namespace puppet {
constexpr int NJ = 34, O_G = 1696, O_W = 704, O_CMP = 176, ND = 22;
// sj_list: pose set, joint, kind (1..3 prismatic x y z, 4..6 rotary) of local-transform lane l
constexpr int N_SJ = 54;
const int sj[N_SJ][3] = {{0,3,6},{0,4,5},{0,5,4},{0,18,6},{0,19,5},{0,20,4},{0,21,4},{0,22,6},{0,23,5},{0,24,4},{0,25,4},{0,26,6},{0,27,5},{0,28,4},{0,29,4},{0,30,6},{0,31,5},{0,32,4},
    {0,33,4},{1,3,6},{1,4,5},{1,5,4},{1,18,6},{1,19,5},{1,20,4},{1,22,6},{1,23,5},{1,24,4},{1,26,6},{1,27,5},{1,28,4},{1,29,4},{1,30,6},{1,31,5},{1,32,4},{1,33,4},
    {0,0,1},{0,1,2},{0,2,3},{1,0,1},{1,1,2},{1,2,3},{1,6,1},{1,7,2},{1,8,1},{1,9,2},{1,10,1},{1,11,2},{1,12,1},{1,13,2},{1,14,1},{1,15,2},{1,16,1},{1,17,2}};
// wev_lane word 3 of config lane l: joint, kind, subtree group
const int cfg[ND][3] = {{0,1,0},{1,2,0},{2,3,0},{3,6,0},{4,5,0},{5,4,0},{18,6,1},{19,5,1},{20,4,1},{21,4,2},{22,6,3},{23,5,3},{24,4,3},{25,4,4},{26,6,5},{27,5,5},{28,4,5},{29,4,6},
    {30,6,7},{31,5,7},{32,4,7},{33,4,8}};
const int b_anchor[10] = {5, 20, 21, 24, 25, 5, 28, 29, 32, 33};
const int ae[12] = {5, 7, 5, 9, 29, 11, 33, 13, 20, 15, 24, 17};      // anchor joint of end point e (lane 3 e + r reads row r)
// dhr_pack: joint of Dh2 record n (its kind is the joint's)
constexpr int N_DHR = 50;
const int dhr[N_DHR] = {0,1,2,3,4,5, 0,1,2,3,4,5, 0,1,2,3,4,5, 26,27,28,29, 0,1,2,3,4,5, 30,31,32,33, 0,1,2,3,4,5, 18,19,20, 0,1,2,3,4,5, 22,23,24};
// the second sweep plan (tr_inst / tr_sched): instances (pose set, first joint) of each pass
const int pass_n[3] = {2, 5, 3};
const int pass_inst[3][5][2] = {{{0,3},{1,3}}, {{0,18},{1,18},{0,22},{1,22},{0,26}}, {{1,26},{0,30},{1,30}}};
inline int kind_of(int j) { for (int i = 0; i < N_SJ; i++) if (sj[i][1] == j) return sj[i][2]; return 1; }
inline int axis(int kind) { return kind >= 4 ? kind - 4 : kind - 1; }
// element (r, c) of joint j in pose set `set`: the 12-double record, and the two arrays of 6-double half-records split by column
inline int at(bool split, int set, int j, int r, int c) {
    const int base = set ? O_W : O_G;
    return split ? base + 6 * j + (c >> 1) * 6 * NJ + 2 * r + (c & 1) : base + 12 * j + 4 * r + c;
}
}  // namespace puppet

int main() {
    double *out; hipMalloc(&out, 64 * 8);
    int ha[64], hb[64];
    // config pairs (a, b) as the composite form lists them: 22 diagonal ones, then ancestors of each config along its path
    for (int i = 0; i < 64; i++) { ha[i] = i < 22 ? i : (i - 22) % 6; hb[i] = i < 22 ? i : 6 + (i - 22) / 6; }
    int *da, *db; hipMalloc(&da, 256); hipMalloc(&db, 256);
    hipMemcpy(da, ha, 256, hipMemcpyHostToDevice); hipMemcpy(db, hb, 256, hipMemcpyHostToDevice);
    const dim3 g(2048), t(64);
    const size_t lds = 19520;
#define RUN(k, ...) hipLaunchKernelGGL(k, g, t, lds, 0, __VA_ARGS__); hipDeviceSynchronize();
    RUN((w_b64<1>), out)      // 1  consecutive doubles (reference)
    RUN((w_b64<6>), out)      // 2  item stride (J, W, X stores)
    RUN((w_b64<12>), out)     // 3  joint stride (local transforms), config stride of the twists
    RUN((w_b64<29>), out)     // 4  image rows
    RUN((w_b128<6>), out)     // 5
    RUN((w_b128<12>), out)    // 6
    RUN((r_b64<1>), out)      // 7
    RUN((r_b64<6>), out)      // 8
    RUN((r_b64<12>), out)     // 9
    RUN((r_b64<29>), out)     // 10
    RUN((r_2b64<6>), out)     // 11
    RUN((r_2b64<12>), out)    // 12
    RUN((r_b128<6>), out)     // 13
    RUN((r_b128<12>), out)    // 14
    RUN(w_quad, out, 0)       // 15
    RUN(w_quad, out, 1)       // 16
    RUN(r_gather, out, da, 12, 1)   // 17 twists of a, 16-byte reads
    RUN(r_gather, out, db, 15, 0)   // 18 per-config vectors of b, 8-byte reads (15-double records are not 16-byte aligned)
    RUN(r_gather, out, da, 12, 0)   // 19
    // round 5: the strides the round-4 verdict asked about for 12-double records (poses, twists): 14 doubles keeps 16-byte alignment, 13 does not
    RUN((w_b64<13>), out)     // 20
    RUN((w_b64<14>), out)     // 21
    RUN((w_b128<14>), out)    // 22
    RUN((r_b64<13>), out)     // 23
    RUN((r_b64<14>), out)     // 24
    RUN((r_2b64<14>), out)    // 25
    RUN((r_b128<14>), out)    // 26
    // pose records of the puppet, lane by lane: every pattern in the 12-double layout, then as two arrays of 6-double half-records split
    // by column; composite records 16 and 18 doubles apart (dispatches 27 .. 72, names in tools/gpu_lds_conflicts.sh)
    {
        using namespace puppet;
        int *dm; hipMalloc(&dm, 256);
        int m[64];
        auto clear = [&]() { for (int l = 0; l < 64; l++) m[l] = -1; };
        auto up = [&]() { hipMemcpy(dm, m, 256, hipMemcpyHostToDevice); };
        for (int pat = 0; pat < 4; pat++)          // local-transform stores: columns a, b, c of the joint's axis order and the translation, row 0
            for (int split = 0; split < 2; split++) {
                clear();
                for (int l = 0; l < N_SJ; l++) { const int a = axis(sj[l][2]); m[l] = at(split, sj[l][0], sj[l][1], 0, pat == 3 ? 3 : (a + pat) % 3); }
                up(); RUN(w_map64, out, dm)
            }
        for (int pat = 0; pat < 2; pat++)          // E3 config lanes: axis column, translation column (the two lanes without a config read joint 0)
            for (int split = 0; split < 2; split++) {
                clear();
                for (int l = 0; l < ND; l++) m[l] = at(split, 0, cfg[l][0], 0, pat ? 3 : axis(cfg[l][1]));
                m[62] = m[63] = at(split, 0, 0, 0, pat ? 3 : 0);
                up(); RUN(r_map64, out, dm)
            }
        for (int split = 0; split < 2; split++) {  // E3 body lanes: a 16-byte word of the anchor joint's pose
            clear();
            for (int b = 0; b < 10; b++) for (int r = 0; r < 3; r++) m[ND + 3 * b + r] = at(split, 0, b_anchor[b], 0, 0);
            up(); RUN(r_map128, out, dm)
        }
        for (int split = 0; split < 2; split++) {  // E3 end points: row r of the anchor joint's q2 pose, first 16-byte word
            clear();
            for (int l = 0; l < 36; l++) m[l] = at(split, 1, ae[l / 3], l % 3, 0);
            up(); RUN(r_map128, out, dm)
        }
        for (int pat = 0; pat < 2; pat++)          // E4 Dh2 records: axis column, translation column of the q2 pose
            for (int split = 0; split < 2; split++) {
                clear();
                for (int l = 0; l < N_DHR; l++) m[l] = at(split, 1, dhr[l], 0, pat ? 3 : axis(kind_of(dhr[l])));
                up(); RUN(r_map64, out, dm)
            }
        for (int ps = 0; ps < 3; ps++)             // chain rounds, lane (instance q, row r, column c): column loads (rows 0 | 1, row 2), parent read, store
            for (int pat = 0; pat < 4; pat++)
                for (int split = 0; split < 2; split++) {
                    clear();
                    for (int l = 0; l < 60; l++) {
                        const int q = l / 12, r = (l % 12) >> 2, c = l & 3;
                        const int parent = ps == 0 ? 2 : 5;     // (round 0 hangs off the last run joint of the torso, round 1 off the torso)
                        if (q < pass_n[ps]) m[l] = at(split, pass_inst[ps][q][0], pat == 2 ? parent : pass_inst[ps][q][1], pat == 0 ? 0 : (pat == 1 ? 2 : r), c);
                    }
                    up();
                    if (pat == 0) { if (split) { RUN((r_map2x64<2>), out, dm) } else { RUN((r_map2x64<4>), out, dm) } }
                    else if (pat == 3) { RUN(w_map64, out, dm) }
                    else { RUN(r_map64, out, dm) }
                }
        for (int stride = 16; stride <= 18; stride += 2) {     // composite records: config lane l reads a 16-byte word of its group's record
            clear();
            for (int l = 0; l < ND; l++) m[l] = O_CMP + stride * cfg[l][2];
            up(); RUN(r_map128, out, dm)
        }
    }
    printf("done: %d repetitions x 2048 waves per pattern\n", REPS);
    return 0;
}
