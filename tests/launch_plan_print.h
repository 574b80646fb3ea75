// One text line per launch of an op-list replay: the launcher, the ops it covers, the requested / resolved tile and family, and
// every field of its argument struct.  A pointer prints as owner+byte offset; the owners are registered by whoever made the
// addresses up (tests/launch_plan_main.cpp; the scratch recorder of tests/test_launch_plan_host.py over a parent commit's engine,
// whose launch_* stand-ins print through this same file — which is what makes the two texts comparable).
#pragma once
#include "kernels.h"

#include <cstdio>
#include <string>
#include <vector>

namespace lp {
using namespace padel;

struct Region { const char* name; const char* base; size_t bytes; };
inline std::vector<Region>& regions() { static std::vector<Region> r; return r; }      // blob, wr, zeros, flag, netin, fc, arena
inline std::vector<const char*>& bufs() { static std::vector<const char*> b; return b; }      // the lane's bptr

// "null" | "buf<k>+0": an activation buffer's base (the lowest k at that address, where buffers share bytes) | "<region>+<bytes>"
inline std::string own(const void* ptr) {
    const char* p = (const char*)ptr;
    if (!p) return "null";
    for (size_t k = 0; k < bufs().size(); ++k)
        if (bufs()[k] == p) return "buf" + std::to_string(k) + "+0";
    for (const Region& r : regions())
        if (p >= r.base && p < r.base + r.bytes) return std::string(r.name) + "+" + std::to_string((size_t)(p - r.base));
    return "unknown";
}
#define LP_P(f) printf(" " #f "=%s", own(a.f).c_str())
#define LP_I(f) printf(" " #f "=%d", (int)a.f)
#define LP_U(f) printf(" " #f "=%u", (unsigned)a.f)

inline void head(const char* launcher, int op, int n_ops) { printf("%s op=%d n=%d", launcher, op, n_ops); }
inline void conv_fields(const ConvArgs& a) {
    LP_P(in); LP_P(w); LP_P(w3); LP_P(bias); LP_P(res); LP_I(res_pre); LP_P(zeros); LP_P(in2); LP_I(in2_cs); LP_I(in2_choff); LP_I(up_c); LP_P(out);
    LP_I(in_cs); LP_I(in_choff); LP_I(out_cs); LP_I(out_choff); LP_I(res_cs); LP_I(res_choff); LP_I(H); LP_I(W); LP_I(Ho); LP_I(Wo); LP_I(cin);
    LP_I(cout); LP_I(n16); LP_I(ksize); LP_I(stride); LP_I(act); LP_I(M); LP_I(n_mtiles); LP_I(n_ntiles); LP_I(tune); LP_I(tap_pd); LP_I(out_f32);
    LP_P(oscale); LP_P(ovf_flag); LP_I(w_single); LP_P(wr); LP_P(dbg); LP_U(howo_magic); LP_U(howo_shift); LP_U(wo_magic); LP_U(wo_shift);
}
inline void stem_fields(const StemArgs& a) {
    LP_P(in); LP_P(w); LP_P(bias); LP_P(out); LP_I(out_cs); LP_I(out_choff); LP_I(H); LP_I(W); LP_I(Ho); LP_I(Wo); LP_I(cout); LP_I(B); LP_I(out_f16);
    LP_P(ovf_flag); LP_U(howo_magic); LP_U(howo_shift); LP_U(wo_magic); LP_U(wo_shift); LP_P(opw);
}
inline void conv(int op, int path, int requested, const ConvLaunched& ran, const ConvArgs& a) {
    head("conv", op, 1);
    printf(" path=%d req=%d ran=%d fam=%s |", path, requested, ran.tile, ran.family);
    conv_fields(a);
    printf("\n");
}
inline void stem(int op, const StemArgs& a) { head("stem", op, 1); printf(" |"); stem_fields(a); printf("\n"); }
inline void stem_l1(int op, const StemArgs& st, const ConvArgs& a) {
    head("stem_l1_h2", op, 2);
    printf(" |");
    stem_fields(st);
    printf(" |");
    conv_fields(a);
    printf("\n");
}
inline void sppf(int op, const float* buf, int cs, int choff, int c, int B, int H, int W, int f16, int fused) {
    head("sppf_pool", op, 1);
    printf(" | buf=%s cs=%d choff=%d c=%d B=%d H=%d W=%d f16=%d fused=%d\n", own(buf).c_str(), cs, choff, c, B, H, W, f16, fused);
}
inline void resize(const char* launcher, int op, const float* in, int in_cs, int in_choff, const float* out, int out_cs, int out_choff, int c, int B,
                   int H, int W, int f16) {          // upsample2x, maxpool2
    head(launcher, op, 1);
    printf(" | in=%s in_cs=%d in_choff=%d out=%s out_cs=%d out_choff=%d c=%d B=%d H=%d W=%d f16=%d\n", own(in).c_str(), in_cs, in_choff, own(out).c_str(),
           out_cs, out_choff, c, B, H, W, f16);
}
inline void maxpool3s2(int op, const float* in, int in_cs, int in_choff, const float* out, int out_cs, int out_choff, int c, int B, int H, int W, int Ho,
                       int Wo, int h2) {
    head("maxpool3s2", op, 1);
    printf(" | in=%s in_cs=%d in_choff=%d out=%s out_cs=%d out_choff=%d c=%d B=%d H=%d W=%d Ho=%d Wo=%d h2=%d\n", own(in).c_str(), in_cs, in_choff,
           own(out).c_str(), out_cs, out_choff, c, B, H, W, Ho, Wo, h2);
}
inline void stem7(int op, const Stem7Args& a) {
    head("stem7", op, 1);
    printf(" |");
    LP_P(in); LP_P(w); LP_P(bias); LP_P(lut); LP_P(out); LP_I(out_cs); LP_I(out_choff); LP_I(H); LP_I(W); LP_I(Ho); LP_I(Wo); LP_I(B); LP_I(act); LP_I(out_h2);
    LP_P(ovf_flag); LP_U(howo_magic); LP_U(howo_shift); LP_U(wo_magic); LP_U(wo_shift);
    printf("\n");
}
inline void gap_fc(int op, const float* in, int in_cs, int in_choff, int c, int B, int HW, const float* w, const float* bias, int nout, const float* logits,
                   const float* probs, int h2) {
    head("gap_fc", op, 1);
    printf(" | in=%s in_cs=%d in_choff=%d c=%d B=%d HW=%d w=%s bias=%s nout=%d logits=%s probs=%s h2=%d\n", own(in).c_str(), in_cs, in_choff, c, B, HW,
           own(w).c_str(), own(bias).c_str(), nout, own(logits).c_str(), own(probs).c_str(), h2);
}
inline void dwconv3(int op, const DwConvArgs& a) {
    head("dwconv3", op, 1);
    printf(" |");
    LP_P(in); LP_P(w); LP_P(bias); LP_P(res); LP_P(out); LP_I(in_cs); LP_I(in_choff); LP_I(out_cs); LP_I(out_choff); LP_I(res_cs); LP_I(res_choff); LP_I(C);
    LP_I(B); LP_I(H); LP_I(W); LP_I(act); LP_I(h2); LP_I(out_f32); LP_P(ovf_flag);
    printf("\n");
}
inline void psa_attn(int op, const AttnArgs& a) {
    head("psa_attn", op, 1);
    printf(" |");
    LP_P(qkv); LP_P(out); LP_I(cs); LP_I(q_choff); LP_I(k_choff); LP_I(v_choff); LP_I(out_cs); LP_I(out_choff); LP_I(heads); LP_I(kd); LP_I(hd); LP_I(N);
    LP_I(B); printf(" scale=%.9g", (double)a.scale); LP_I(h2); LP_I(out_f32); LP_P(ovf_flag);
    printf("\n");
}

}  // namespace lp
