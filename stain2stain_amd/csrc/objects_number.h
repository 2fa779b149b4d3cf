// The numbering stage of s2s_objects_label, shared with s2s_split_label (split.hip): defined once, in objects.hip.
//
// In:  labels int [B][H][W], labels[i] = the smallest raster index of the set pixel i belongs to (so labels[r] == r at
//      exactly one pixel per set, its first in raster order), negative on pixels of no set.
// Out: labels[i] = the set's number (kept sets, area >= min_area, 1..count in raster order of their first pixel; 0 for
//      the others and for the pixels of no set), count [B] written, kept_pixels / largest / size_hist accumulated into
//      (the caller zeroes them), the rows < min(count, max_objects) of the tables written.
// area:  int [B][H][W] of scratch, any contents; chunk: int [B][ceil(H W / 1024)] of scratch, any contents.
// Six launches on `stream` (zero, area, count, scan, number, relabel); nothing allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>

__attribute__((visibility("hidden"))) long s2s_number_chunks(long hw);
__attribute__((visibility("hidden"))) void s2s_number_sets(int* labels, int* area, int* chunk, int B, int H, int W,
                                                          int min_area, int max_objects, int* count,
                                                          long long* kept_pixels, int* largest, long long* size_hist,
                                                          int* tab_area, int* tab_bbox, long long* tab_sums,
                                                          hipStream_t stream);
