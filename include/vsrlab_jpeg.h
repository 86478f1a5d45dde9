/* vsrlab_jpeg.h -- C ABI of libvsrlab_jpeg.so: the JPEG round trip of core/augmentations.py RandomJPEGCompression.
 *
 * A library of its own beside libvsrlab_hip.so, whose set of exported symbols is pinned (ABI 4) and stays as it is.  The
 * conventions are those of include/vsrlab_hip.h: device pointers, a hipStream_t passed as void*, 0 (VSR_STATUS_OK) or a negative
 * VSR_STATUS_* code returned, nothing thrown; the status-string call of libvsrlab_hip.so names the codes.  Neither library needs
 * the other to be loaded.                                                                                                      */
#ifndef VSRLAB_JPEG_H
#define VSRLAB_JPEG_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- JPEG compression and decompression of RGB frames in one call (csrc/jpeg_degrade.hip) ---------------
 * What the reference does per frame on a loader CPU -- to_pil_image, libjpeg at `quality` with 4:2:0 chroma, to_tensor -- as the
 * fixed-point specification of DESIGN section 11g: integer arithmetic throughout, bit-identical to PIL / libjpeg-turbo.  No
 * entropy coding happens: it is lossless and leaves the pixels as they are.  Forward only.
 *   x, y: (N, 3, H, W) planar RGB of x_dtype / y_dtype (0: fp32, 1: bf16) with the ELEMENT strides x_stride / y_stride
 *         (n, c, h, w; any non-overlapping layout of y, any layout of x).  x is clamped to [0, 1]; y is one of k / 255.
 *   ws:   workspace_bytes(d) bytes, 256-byte aligned, owned by the call until it finished: the decoded Y plane (N, Hp, Wp) and
 *         the decoded Cb and Cr planes (N, Hp / 2, Wp / 2) as bytes, Hp and Wp = H and W rounded up to 16.  These 1.5 bytes
 *         per padded pixel are the only intermediates in memory.
 * Supported: N in 1..65535, H and W in 1..32768, quality any int (clamped to 1..100).  Anything else is
 * VSR_STATUS_UNSUPPORTED (workspace_bytes: 0) before any launch.                                                               */
typedef struct VsrJpegDesc {
    int N, H, W;
    int quality;
    int x_dtype, y_dtype;
    long long x_stride[4], y_stride[4];
} VsrJpegDesc;
size_t vsr_jpeg_workspace_bytes(const VsrJpegDesc* d);                                  /* 0: unsupported descriptor */
int vsr_jpeg_fwd(const VsrJpegDesc* d, const void* x, void* y, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSRLAB_JPEG_H */
