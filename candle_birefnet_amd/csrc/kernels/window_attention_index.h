// window_attention_index.h — where the relative position bias of a (query, key) pair lies in a head's table column.  Shared by the window
// attention kernels (kernels/window_attention.hip) and a stand-alone CPU check (tests/test_attention_bias_index_cpu.py): plain integer
// arithmetic, no HIP header needed.  WSZ = window side; a token is ti * WSZ + tj, the table has (2 WSZ - 1)^2 entries.
//
// relative position index (swin.rs:182-184) of (query (qi, qj), key (ki, kj)) = (qi - ki + WSZ - 1) (2 WSZ - 1) + (qj - kj + WSZ - 1)
//                                                                            = att_qbase(qi, qj) - (key + (WSZ - 1) (key / WSZ)).
// With the table stored reversed (rev[j] = table[(2 WSZ - 1)^2 - 1 - j]) the index GROWS with the key:
//   rev index = att_qrev(qi, qj) + att_koff(key),   att_koff(key) = key + (WSZ - 1) (key / WSZ),
// and for keys key0 .. key0 + 3 of ONE window row (key0 % 4 == 0 and WSZ % 4 == 0) att_koff(key0 + r) = att_koff(key0) + r: the four
// scores a lane holds of a 16-key tile (keys 16 kt + 4 g + r) read four consecutive words from one address.
#pragma once

#if defined(__HIPCC__)
#define BRN_AI_HD __host__ __device__ __forceinline__
#else
#define BRN_AI_HD inline
#endif

namespace brn {

template <int WSZ = 12>
BRN_AI_HD int att_qbase(int qi, int qj) { return (qi + WSZ - 1) * (2 * WSZ - 1) + qj + WSZ - 1; }
template <int WSZ = 12>
BRN_AI_HD int att_qrev(int qi, int qj) { return (2 * WSZ - 1) * (2 * WSZ - 1) - 1 - att_qbase<WSZ>(qi, qj); }
template <int WSZ = 12>
BRN_AI_HD int att_koff(int key) { return key + (WSZ - 1) * (key / WSZ); }
// first key of the four that lane group g holds of key tile kt (C/D map of the 16x16 MFMA: row = 4 g + reg)
BRN_AI_HD int att_key0(int kt, int g) { return kt * 16 + g * 4; }

}  // namespace brn
