// The plain C-ABI functions of include/s2k.h (the ones that are not stage records): each has a check_* that validates every argument
// on the host without a HIP call, and a launch_* with the same arguments plus the stream.  s2k_api.hip runs the pair through one
// guarded call; the file that defines a pair includes this header, so a prototype cannot drift from its definition.
#pragma once
#include "common.h"

namespace s2k {

// ew.hip
int check_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double b1, double b2, double eps, double wd, int step);
int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double b1, double b2, double eps, double wd, int step,
                hipStream_t st);

// igemm.hip
int check_mfma_selftest(const float* a, const float* b, float* d);
int launch_mfma_selftest(const float* a, const float* b, float* d, hipStream_t st);

// mae_render.hip
int check_mae_panels(const float* imgs, const float* pred, const float* mask, const float* norm, const double* bounds, unsigned char* out,
                     float* patch_mse, int B, int C, int T, int H, int W, int P, int TUB, const int* bands, int frame, const int* panels,
                     int n_panels, int fill, int norm_pix);
int launch_mae_panels(const float* imgs, const float* pred, const float* mask, const float* norm, const double* bounds, unsigned char* out,
                      float* patch_mse, int B, int C, int T, int H, int W, int P, int TUB, const int* bands, int frame, const int* panels,
                      int n_panels, int fill, int norm_pix, hipStream_t st);

// classmap.hip
int check_classmap_filter(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int size,
                          int mode, unsigned votes, unsigned fixed, int ignore, const unsigned char* labels, const int* index, const int* lut,
                          int nsrc, unsigned long long* hist, unsigned long long* changed);
int launch_classmap_filter(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int size,
                           int mode, unsigned votes, unsigned fixed, int ignore, const unsigned char* labels, const int* index, const int* lut,
                           int nsrc, unsigned long long* hist, unsigned long long* changed, hipStream_t st);

// components.hip
int check_classmap_components(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int connectivity, unsigned exclude,
                              int* labels, int* areas, unsigned long long* counts, unsigned* status);
int launch_classmap_components(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int connectivity, unsigned exclude,
                               int* labels, int* areas, unsigned long long* counts, unsigned* status, hipStream_t st);
int check_classmap_sieve(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int min_area,
                         unsigned fixed, int to, const int* labels, const int* areas, unsigned long long* best, const unsigned char* hist_labels,
                         const int* index, const int* lut, int nsrc, unsigned long long* hist, unsigned long long* changed, unsigned* status);
int launch_classmap_sieve(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int min_area,
                          unsigned fixed, int to, const int* labels, const int* areas, unsigned long long* best, const unsigned char* hist_labels,
                          const int* index, const int* lut, int nsrc, unsigned long long* hist, unsigned long long* changed, unsigned* status,
                          hipStream_t st);

// distance.hip
int check_classmap_distance(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int mode, unsigned sites,
                            int connectivity, unsigned exclude, void* work, int* dist2, int* nearest, const void* other, int other_bytes,
                            const int* edges, int n_edges, unsigned long long* hist);
int launch_classmap_distance(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int mode, unsigned sites,
                             int connectivity, unsigned exclude, void* work, int* dist2, int* nearest, const void* other, int other_bytes,
                             const int* edges, int n_edges, unsigned long long* hist, hipStream_t st);
size_t classmap_distance_workspace(int M, int H, int W);

// calibration.hip
int check_calibration(const float* scores, int mode, const void* labels, int label_bytes, const int* label_lut, int N, int K, int P,
                      unsigned exclude, const float* temps, int n_temps, int bins, int measure, float reject_below, int reject_to, float* conf,
                      void* pred, int pred_bytes, unsigned long long* hist, unsigned long long* totals, unsigned long long* skipped);
int launch_calibration(const float* scores, int mode, const void* labels, int label_bytes, const int* label_lut, int N, int K, int P,
                       unsigned exclude, const float* temps, int n_temps, int bins, int measure, float reject_below, int reject_to, float* conf,
                       void* pred, int pred_bytes, unsigned long long* hist, unsigned long long* totals, unsigned long long* skipped,
                       hipStream_t st);

// rasterize.hip
int check_rasterize(const int* verts, int V, const int* ring_start, const int* ring_shape, int R, const int* values, int S, const int* origins,
                    int M, int H, int W, void* dst, int dst_bytes, int mode, int burn, int fill, void* work, long long* unfilled, int* status);
int launch_rasterize(const int* verts, int V, const int* ring_start, const int* ring_shape, int R, const int* values, int S, const int* origins,
                     int M, int H, int W, void* dst, int dst_bytes, int mode, int burn, int fill, void* work, long long* unfilled, int* status,
                     hipStream_t st);
size_t rasterize_workspace(int M, int S);

// zonal.hip
int check_zonal_histogram(const void* zone, int zone_bytes, int zone_stride, const void* cls, int cls_bytes, const int* src_lut, int M, int H,
                          int W, int Z, int K, long long* hist, unsigned* status);
int launch_zonal_histogram(const void* zone, int zone_bytes, int zone_stride, const void* cls, int cls_bytes, const int* src_lut, int M, int H,
                           int W, int Z, int K, long long* hist, unsigned* status, hipStream_t st);
int check_zonal_bands(const void* zone, int zone_bytes, int zone_stride, const short* vals, int M, int C, int H, int W, int Z, int nodata,
                      int has_nodata, long long* count, long long* sum, long long* sumsq, int* mn, int* mx, unsigned* status);
int launch_zonal_bands(const void* zone, int zone_bytes, int zone_stride, const short* vals, int M, int C, int H, int W, int Z, int nodata,
                       int has_nodata, long long* count, long long* sum, long long* sumsq, int* mn, int* mx, unsigned* status, hipStream_t st);
int check_zonal_majority(const long long* hist, int Z, int K, unsigned votes, long long min_count, int fill, int* out_cls, long long* out_best);
int launch_zonal_majority(const long long* hist, int Z, int K, unsigned votes, long long min_count, int fill, int* out_cls, long long* out_best,
                          hipStream_t st);
int check_zonal_paint(const void* zone, int zone_bytes, int zone_stride, const int* table, int M, int H, int W, int Z, void* dst, int dst_bytes,
                      int mode, int fill, unsigned* status);
int launch_zonal_paint(const void* zone, int zone_bytes, int zone_stride, const int* table, int M, int H, int W, int Z, void* dst, int dst_bytes,
                       int mode, int fill, unsigned* status, hipStream_t st);

}  // namespace s2k
