// kernels/gemm_bf16.hip a second time with fp16 as the 16-bit storage type (namespace brn::hf), as the Makefile's -DBRN_S16_F16=1 rule compiles it
#define BRN_S16_F16 1
#include "kernels/gemm_bf16.hip"
