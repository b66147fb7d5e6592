// vr_ingest.h -- launchers of the device-side volume ingest (vr_ingest.hip): what DatRawReader::read_raw
// does per voxel on the host (maximum, USHORT stretch / FLOAT normalisation, 256-bin histogram), on a
// volume that is already in HBM.  Used by vrhip_ingest_raw and vrhip_volume_histogram (vrhip_api.hip).
#pragma once
#include "vr_internal.h"

// The loader's arithmetic for one time step, fixed once the maximum is known.
struct IngestParams {
    float max_value;   // FLOAT: the divisor
    float stretch;     // USHORT: 65535.f / max, computed on the host in fp32
    int big_endian;    // the file's words are big-endian
};

// What the running maximum starts from, in the encoding the max kernel reduces on: FLOAT the bit
// pattern of FLT_MIN (every candidate is a larger positive float, and those order like their bits),
// USHORT 0 (= "no word above FLT_MIN yet").
inline uint32_t vr_ingest_max_init(int format) { return format == VRHIP_FLOAT ? 0x00800000u : 0u; }
// ... and the loader's `maximum` from the reduced word
inline float vr_ingest_max_decode(int format, uint32_t word)
{
    if (format == VRHIP_UCHAR) return 255.f;
    if (format == VRHIP_USHORT) return word ? (float)word : __builtin_bit_cast(float, 0x00800000u);
    return __builtin_bit_cast(float, word);
}

// max_word = max(max_word, words[0 .. n)) with the loader's rules: FLOAT words are byte-swapped first
// when big_endian, USHORT words never; NaN never wins.  `words` is 16-byte aligned and readable up to
// the next multiple of 16 bytes.  UCHAR: nothing to do (the loader's maximum is 255).
hipError_t vr_launch_ingest_max(const void *words, size_t n, int format, int big_endian, uint32_t *max_word,
                                int num_cus, hipStream_t stream);
// In place over the micro-bricked array vol.data (one channel plane), raw words as re-tiled from the
// file: converts every voxel (convert != 0) and counts the voxels inside the volume into hist[256].
// convert == 0: nothing is written, the binning is applied to the stored values as they are.
hipError_t vr_launch_ingest_convert(const VolView &vol, int format, const IngestParams &p, int convert,
                                    unsigned long long *hist, int num_cus, hipStream_t stream);
// The same conversion and count over n words of a flat array (the bytes of a file beyond the volume):
// nothing is written.  Alignment as for vr_launch_ingest_max.
hipError_t vr_launch_ingest_count(const void *words, size_t n, int format, const IngestParams &p,
                                  unsigned long long *hist, int num_cus, hipStream_t stream);
// n_texels interleaved texels of `channels` (2 or 4) values -> one planar array per channel, plane c at
// planar + c * plane_stride elements.  Both 16-byte aligned, plane_stride a multiple of 16 bytes.
hipError_t vr_launch_deinterleave(const void *interleaved, void *planar, size_t plane_stride, size_t n_texels,
                                  int format, int channels, hipStream_t stream);
