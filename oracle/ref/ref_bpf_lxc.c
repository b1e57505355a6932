/* bpf_lxc.c of the reference as host code: the helper declarations of api.h
 * become plain prototypes, ref_shim.h defines them.  Nothing else lives here. */
#define BPF_FUNC(NAME, ...) NAME(__VA_ARGS__)
#include "bpf_lxc.c"
#include "ref_shim.h"
