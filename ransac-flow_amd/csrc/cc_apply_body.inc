// Body of the apply kernels (cc.hip).  The including kernel has set in, label, area, out (at the first pixel it owns), total,
// max_area and HW = the pixels of one image.
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int l = label[i];
        // a component that IS the whole image is never removed: the reference walks np.unique(label)[1:], taking the first id
        // for the background, and returns early when there is only one id (evaluation/evalKITTI/evaluation.py:90-93)
        const int a = l >= 0 ? area[l] : 0;
        out[i] = (l >= 0 && a <= max_area && a < HW) ? 0.0f : in[i];
    }
