# asan_ring.mk -- the device entry ring's check program (tests/cpp/host_ring_check.cpp over
# include/fi_ring.h) under AddressSanitizer + UBSan, built beside the product like tsan.mk's
# programs and with the same host-only instrumentation (no GPU sanitizer):
#   make -f tests/cpp/asan_ring.mk   (from the repository root, after `make`;
#                                     __graft_entry__.build() runs it)
# The program links a library of its own, build/asan_ring/lib/libfi_learner.so: the host sides of
# csrc/ring.hip (the handle, its counters and every refusal) and csrc/learner.cpp instrumented, the
# product's device objects and the actor, rollout and gather objects as `make` left them. The
# program needs the device (it creates actors and a learner), so this recipe only builds it; it is
# a stand-alone program and takes no preloaded runtime.
CLANGXX ?= /opt/rocm/lib/llvm/bin/clang++
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := freeimpala_amd/csrc
OUT := build/asan_ring
RLIB := $(OUT)/lib
OBJS := $(patsubst %,build/obj/%.hip.o,farmer vtrace gemm_f32 misc atari atari_fr fc_gemm actor rollout gather)
ASAN_HIP := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=all
HIPFLAGS := --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Iinclude -I$(CSRC) -Wno-unused-value -Wno-unused-result $(ASAN_HIP)
CHDRS := $(wildcard $(CSRC)/*.h) $(wildcard include/*.h)

all: $(OUT)/host_ring_check

$(OUT)/learner.cpp.o: $(CSRC)/learner.cpp $(CHDRS)
	@mkdir -p $(OUT)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(OUT)/ring.hip.o: $(CSRC)/ring.hip $(CHDRS)
	@mkdir -p $(OUT)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(RLIB)/libfi_learner.so: $(OUT)/learner.cpp.o $(OUT)/ring.hip.o $(OBJS)
	@mkdir -p $(RLIB)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $^ -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

$(OUT)/host_ring_check: tests/cpp/host_ring_check.cpp $(wildcard include/freeimpala_amd/*.hpp) $(wildcard include/*.h) $(RLIB)/libfi_learner.so
	@mkdir -p $(OUT)
	$(CLANGXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude $< -o $@ -pthread -L$(RLIB) -lfi_learner '-Wl,-rpath,$$ORIGIN/lib' -Wl,-rpath,/opt/rocm/lib

.PHONY: all
