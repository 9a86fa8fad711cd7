// Eligibility test + dispatcher for the k-means step's cell kernel (see xna_kmeans_kernel.h); gather and mass reduction are mask pooling's.
#include "xna_kmeans_kernel.h"

// the instances: xna_kmeans_inst.hip, one object per window
#define NAF_X(K) NAF_XNA_KMEANS_WINDOW(extern, K)
NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X

// NAF_OK when the kernel serves the (validated) request; otherwise NAF_ERR_UNSUPPORTED with the reason in the error string.
int naf_xna_kmeans_eligible(const naf_xna_kmeans_args* a) {
    const int rc = xna_headsum_shape_eligible("naf_xna_kmeans", a);
    if (rc != NAF_OK) return rc;
    if (a->K > 64) {
        naf_set_error("naf_xna_kmeans: the fused kernel takes at most 64 clusters (got %d)", a->K);
        return NAF_ERR_UNSUPPORTED;
    }
    if (!xna_qkv_layout_ok(a, a->pv_lr, a->pv_stride)) {   // which half of it
        if (!naf_aligned(a->q, 16) || !naf_aligned(a->k_lr, 16) || !naf_aligned(a->pv_lr, 16)) naf_set_error("naf_xna_kmeans: the fused kernel needs 16-byte aligned q, k_lr, pv_lr");
        else naf_set_error("naf_xna_kmeans: the fused kernel needs q / k_lr / pv_lr strides that are multiples of 8 elements");
        return NAF_ERR_UNSUPPORTED;
    }
    return NAF_OK;
}

int naf_launch_xna_kmeans(const naf_xna_kmeans_args* a, float scale, hipStream_t s) {
    XnaKmeansParams p;
    xna_fill_common(p, a, a->pv_stride, scale);
    size_t moff = 0;
    naf_xna_pool_ws(a->B, a->heads, a->h, a->w, a->ky * a->kx, a->K, &moff);
    p.pv = static_cast<const bf16_t*>(a->pv_lr);
    p.bias = a->bias;
    p.bias_stride_b = a->bias_stride_b;
    p.labels = a->labels;
    p.part = static_cast<float*>(a->workspace);
    p.pmass = reinterpret_cast<float*>(static_cast<char*>(a->workspace) + moff);
    p.tab_y = a->rope_tab_y; p.tab_x = a->rope_tab_x;
    p.dy = a->Ho / a->h; p.dx = a->Wo / a->w;
    p.K = a->K;
    p.kpad = (a->K + 15) & ~15;
    for (int i = 0; i < 3; ++i) p.ls[i] = a->labels_stride[i];
    int rc = xna_grid("naf_xna_kmeans_fwd", (int64_t)a->B * a->h * a->w, &p.nblocks);
    if (rc != NAF_OK) return rc;
    rc = NAF_ERR_UNSUPPORTED;
    switch (a->ky) {
#define NAF_X(K) case K: rc = xna_kmeans_launch_ks<K>(p, a->A, s); break;
        NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
        default: naf_set_error("naf_xna_kmeans_fwd: kernel size %d has no instantiation", a->ky);
    }
    if (rc != NAF_OK) return rc;
    return naf_launch_xna_pool_mass(p.pmass, a->mass, a->B, a->K, p.kpad, a->h * a->w, s);
}
