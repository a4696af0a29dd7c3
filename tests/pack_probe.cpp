// Host program of tests/test_pack_cpu.py: builds the device weight image (csrc/sm_pack.h) of one model without a GPU.
//   pack_probe IN OUT   IN = shapemol_config (10 x int32) followed by the packed float32 weights; OUT receives the image bytes.
// Prints "name value" lines: the image size in floats, hid_max and every offset of DevModel / DevLayer.
#include "../shapemol_amd/csrc/sm_pack.h"

#include <cstdio>

#define P(obj, f) std::printf("%s." #f " %zu\n", pre.c_str(), (size_t)(obj).f)
static void show(const std::string &pre, const DevMlp &d) { P(d, w1); P(d, b1); P(d, g); P(d, be); P(d, w2); P(d, b2); }
static void show(const std::string &pre, const DevMlpImg &d) {
    P(d, w1img); P(d, b1); P(d, g); P(d, be); P(d, w2img); P(d, b2); P(d, nt2); P(d, w1img6); P(d, w2img6); P(d, w1img16); P(d, w2img16);
}
static void show(const std::string &pre, const DevLayer &d) {
    P(d, pre_x2h); P(d, pre_h2x); P(d, lin_img); P(d, lin6_img); P(d, pre6_x2h); P(d, lin16_img); P(d, pre16_x2h);
    P(d, sk_x2h); P(d, sv_x2h); P(d, sk_h2x); P(d, sv_h2x); P(d, bk_x2h); P(d, bv_x2h); P(d, bk_h2x); P(d, bv_h2x);
    show(pre + ".q_x2h", d.q_x2h); show(pre + ".q_h2x", d.q_h2x); show(pre + ".no", d.no);
    P(d, blob_x2h); P(d, blob_h2x); P(d, img_kx); P(d, img_vx); P(d, img_kh); P(d, img_vh);
    P(d, i16_kx); P(d, i16_vx); P(d, i16_kh); P(d, i16_vh); P(d, st_kx); P(d, st_vx); P(d, st_kh); P(d, st_vh);
    P(d, sw2_kx); P(d, sw2_vx); P(d, sw2_kh); P(d, sb2_vx); P(d, vn_f); P(d, vn_d);
    P(d, wf_x); P(d, wd_x); P(d, wf_o); P(d, wd_o); P(d, bn_g); P(d, bn_b);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    shapemol_config cfg;
    if (!f || std::fread(&cfg, sizeof(cfg), 1, f) != 1) return 2;
    std::vector<float> w(weight_count(cfg));
    if (std::fread(w.data(), sizeof(float), w.size(), f) != w.size() || std::fgetc(f) != EOF) return 2;
    std::fclose(f);
    HostModel hm;
    Image im;
    DevModel dm;
    float hid_max = 0.f;
    if (!parse_weights(cfg, w.data(), w.size(), hm) || build_model_image(cfg, hm, im, dm, hid_max)) {
        std::fprintf(stderr, "%s\n", g_err.c_str());
        return 1;
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(im.d.data(), sizeof(float), im.d.size(), f) != im.d.size() || std::fclose(f)) return 2;
    std::printf("size %zu\nhid_max %.9g\n", im.d.size(), (double)hid_max);
    const std::string pre = "dm";
    for (int i = 0; i < 7; ++i) std::printf("dm.tab%d %zu\n", i, dm.tab[i]);
    P(dm, te1w); P(dm, te1b); P(dm, te2w); P(dm, te2b); P(dm, embw); P(dm, embb); P(dm, embwT);
    show("dm.ew", dm.ew); show("dm.inv", dm.inv); show("dm.vhead", dm.vhead);
    for (size_t l = 0; l < dm.layer.size(); ++l) show("dm.layer" + std::to_string(l), dm.layer[l]);
    return 0;
}
