// Packed conv-weight images: W[co][ci][tap] gathered from the raw weight (w_base / w_sco / w_sci / w_stap addressing) into the
// order a conv kernel consumes it, zero padded.  Each layout is written once: set_fill_pack_desc (host) holds its padding rule,
// one device function maps an image element to (co, ci, tap), pack_element gathers and stores.  The same kernel body serves the
// per-image entries (one descriptor by value) and the optimizer's one-launch re-pack of every image (a descriptor table on the
// device: ~100 - 170 pack launches of ~5 us per training step otherwise, 1.1 ms of a 32 ms fp32 step on the compute stream).
#include "weight_image.h"

namespace {

struct WIdx {
    int co, ci, tap;
};

// SET_IMG_F32:  wp[rb][tap][cp][lane] = W[32 rb + (lane & 31)][2 cp + (lane >> 5)][tap]   (MFMA A-fragment order)
__device__ __forceinline__ WIdx img_f32_index(const SetPackDesc &e, int64_t idx) {
    const int lane = (int)(idx & 63);
    int64_t r = idx >> 6;
    const int cp_total = e.CinP / 2;
    const int cp = (int)(r % cp_total);
    r /= cp_total;
    const int tap = (int)(r % e.K);
    const int rb = (int)(r / e.K);
    return {rb * 32 + (lane & 31), 2 * cp + (lane >> 5), tap};
}

// SET_IMG_F32_BIG:  wp[g][w][ks][lane][rb] = W[row][ci][tap],  row = g*128*RB + w*32*RB + rb*32 + (lane&31),
// ks enumerates (chunk, tap, channel pair) in the kernel's consumption order, ci = chunk0 + 2*cp + (lane>>5)
__device__ __forceinline__ WIdx img_f32_big_index(const SetPackDesc &e, int64_t idx) {
    const int rb = (int)(idx % e.RB);
    const int lane = (int)((idx / e.RB) & 63);
    int64_t r = idx / e.RB / 64;
    const int64_t ks_total = (int64_t)e.K * (e.CinP / 2);
    int64_t ks = r % ks_total;
    r /= ks_total;
    const int wv = (int)(r & 3), g = (int)(r >> 2);
    const int co = g * 128 * e.RB + wv * 32 * e.RB + rb * 32 + (lane & 31);
    int c0 = 0;
    for (;;) {  // ks -> (chunk, tap, cp)
        const int CH = e.CinP - c0 < e.ch_max ? e.CinP - c0 : e.ch_max;
        const int64_t per_chunk = (int64_t)e.K * (CH / 2);
        if (ks < per_chunk) return {co, c0 + 2 * (int)(ks % (CH / 2)) + (lane >> 5), (int)(ks / (CH / 2))};
        ks -= per_chunk;
        c0 += CH;
    }
}

// SET_IMG_BF16:  wp[tap][chunk][row][32]   (row < CoutP, chunk < CinP / 32)
// One (tap, chunk, 64..128-row block) is a contiguous run of 64-byte rows: a block copies it to LDS with 16-byte units.
__device__ __forceinline__ WIdx img_bf16_index(const SetPackDesc &e, int64_t idx) {
    const int kk = (int)(idx & 31);
    int64_t r = idx >> 5;
    const int row = (int)(r % e.CoutP);
    r /= e.CoutP;
    const int nchunk = e.CinP / 32;
    const int chunk = (int)(r % nchunk);
    return {row, chunk * 32 + kk, (int)(r / nchunk)};
}

__device__ __forceinline__ void pack_element(const SetPackDesc &e, int64_t idx) {
    const WIdx i = e.kind == SET_IMG_F32 ? img_f32_index(e, idx) : e.kind == SET_IMG_F32_BIG ? img_f32_big_index(e, idx) : img_bf16_index(e, idx);
    float v = 0.0f;
    if (i.co < e.Cout && i.ci < e.Cin) v = e.w[e.w_base + (int64_t)i.co * e.w_sco + (int64_t)i.ci * e.w_sci + (int64_t)i.tap * e.w_stap];
    if (e.kind == SET_IMG_BF16) reinterpret_cast<unsigned short *>(e.wp)[idx] = f2bf(v);
    else reinterpret_cast<float *>(e.wp)[idx] = v;
}

// where the descriptor of element gidx comes from: the kernel argument itself, or a table sorted by `start`
struct PackOne {
    SetPackDesc e;
    __device__ const SetPackDesc &at(int64_t) const { return e; }
};
struct PackTable {
    const SetPackDesc *d;
    int n;
    __device__ SetPackDesc at(int64_t gidx) const {
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (d[mid].start <= gidx) lo = mid; else hi = mid - 1;
        }
        return d[lo];
    }
};

template <typename Src>
__global__ void __launch_bounds__(256) pack_conv_weight_kernel(Src src, int64_t total) {
    const int64_t gidx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gidx >= total) return;
    const SetPackDesc e = src.at(gidx);
    pack_element(e, gidx - e.start);
}

int pack_one(const char *what, int kind, const float *w, void *wp, int Cout, int Cin, int K, int dil, int64_t w_base, int64_t w_sco,
             int64_t w_sci, int64_t w_stap, void *stream) {
    SET_REQUIRE(w && wp && Cout > 0 && Cin > 0 && K > 0, what);
    PackOne one = {{w, wp, w_base, w_sco, w_sci, w_stap, /*start*/ 0, Cout, Cin, K}};
    const int64_t total = set_fill_pack_desc(&one.e, kind, dil);
    hipLaunchKernelGGL(pack_conv_weight_kernel<PackOne>, dim3(set_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, one, total);
    return set_check_launch(what);
}

int64_t image_size(int kind, int Cout, int Cin, int K) {
    SetPackDesc d = {nullptr, nullptr, 0, 0, 0, 0, 0, Cout, Cin, K};
    return set_fill_pack_desc(&d, kind, 0);
}

}  // namespace

extern "C" int64_t set_sizeof_pack_desc(void) { return (int64_t)sizeof(SetPackDesc); }

// the padding rules of the three layouts: kind, CinP, CoutP, RB, ch_max from Cout / Cin / K (and |dil| for the big-tile image)
extern "C" int64_t set_fill_pack_desc(SetPackDesc *d, int32_t kind, int32_t dil) {
    if (d == nullptr || kind < SET_IMG_F32 || kind > SET_IMG_BF16 || d->Cout <= 0 || d->Cin <= 0 || d->K <= 0) return -1;
    d->kind = kind;
    d->RB = 1;
    d->ch_max = 0;
    if (kind == SET_IMG_F32) {
        d->CoutP = set_round_up(d->Cout, 32);
        d->CinP = set_round_up(d->Cin, KC);
    } else if (kind == SET_IMG_F32_BIG) {
        d->RB = v2_rb(d->Cout);
        d->ch_max = v2_ch_max((d->K - 1) * (dil < 0 ? -dil : dil));
        d->CoutP = set_round_up(d->Cout, 128 * d->RB);
        d->CinP = set_round_up(d->Cin, V2_CIN_PAD);
    } else {
        d->CoutP = set_round_up(d->Cout, BF16_IMG_ROWS);
        d->CinP = set_round_up(d->Cin, BF16_IMG_CH);
    }
    return (int64_t)d->CoutP * d->K * d->CinP;
}

extern "C" int64_t set_packed_conv_weight_size(int32_t Cout, int32_t Cin, int32_t K) { return image_size(SET_IMG_F32, Cout, Cin, K); }
extern "C" int64_t set_packed_conv_weight_v2_size(int32_t Cout, int32_t Cin, int32_t K) { return image_size(SET_IMG_F32_BIG, Cout, Cin, K); }
extern "C" int64_t set_packed_conv_weight_bf16_size(int32_t Cout, int32_t Cin, int32_t K) { return image_size(SET_IMG_BF16, Cout, Cin, K); }

extern "C" int set_pack_conv_weight(const float *w, float *wp, int32_t Cout, int32_t Cin, int32_t K, int64_t w_base, int64_t w_sco,
                                    int64_t w_sci, int64_t w_stap, void *stream) {
    return pack_one("set_pack_conv_weight", SET_IMG_F32, w, wp, Cout, Cin, K, 0, w_base, w_sco, w_sci, w_stap, stream);
}
extern "C" int set_pack_conv_weight_v2(const float *w, float *wp, int32_t Cout, int32_t Cin, int32_t K, int32_t dil, int64_t w_base,
                                       int64_t w_sco, int64_t w_sci, int64_t w_stap, void *stream) {
    return pack_one("set_pack_conv_weight_v2", SET_IMG_F32_BIG, w, wp, Cout, Cin, K, dil, w_base, w_sco, w_sci, w_stap, stream);
}
extern "C" int set_pack_conv_weight_bf16(const float *w, void *wp, int32_t Cout, int32_t Cin, int32_t K, int64_t w_base, int64_t w_sco,
                                         int64_t w_sci, int64_t w_stap, void *stream) {
    return pack_one("set_pack_conv_weight_bf16", SET_IMG_BF16, w, wp, Cout, Cin, K, 0, w_base, w_sco, w_sci, w_stap, stream);
}

extern "C" int set_pack_conv_weights_batch(const SetPackDesc *descs_dev, int32_t n, int64_t total, void *stream) {
    SET_REQUIRE(descs_dev && n > 0 && total > 0, "set_pack_conv_weights_batch");
    hipLaunchKernelGGL(pack_conv_weight_kernel<PackTable>, dim3(set_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       PackTable{descs_dev, n}, total);
    return set_check_launch("set_pack_conv_weights_batch");
}
