# Build of the MI355X base64 byte-stream engine and its test oracle.
#
#   make            -> async_amd/libasync_b64.so  (product: HIP kernels + C ABI
#                      + host-only sessions/lanes unit + bytestream_1 stages
#                      + minimal loop/streams)
#                      oracle/liboracle.so          (test infrastructure only)
#                      tests/csrc/libstage_harness.so, libstage_fake.so,
#                      libb64x_hooks.so     (test infrastructure only)
#   make clean
#
# Everything is compiled for gfx950 only (no other offload targets, no
# CUDA/HIP dual path).  Code object v5 keeps the library loadable by both
# the ROCm 7.2 runtime of this image and the ROCm 7.0 runtime bundled with
# the PyTorch wheel (the Python side imports torch first, see
# async_amd/_lib.py).

HIPCC    ?= /opt/rocm/bin/hipcc
CC       ?= gcc
ARCH     ?= gfx950
# -Wno-pass-failed: k_encode_flat's `#pragma unroll` loops (compile-time trip
# counts) are reported "not unrolled" after they have already been fully
# unrolled by an earlier pass; the ISA is the unrolled one.
# -amdgpu-kernarg-preload-count: the first 16 dwords of kernel arguments
# arrive in SGPRs, so a wave's first address needs no kernarg load (encode
# -2 us, CRLF-76 decode -2.5 us per 1 GiB in A/B; the code object keeps the
# loading prologue for firmware without preload).
HIPFLAGS  = --offload-arch=$(ARCH) -mcode-object-version=5 -O3 -std=c++17 -fPIC -Iasync_amd/csrc \
            -Wall -Wno-pass-failed -Iinclude -mllvm -amdgpu-kernarg-preload-count=16
# The host-only C++ unit: the same language level and warnings, no offload
# (as plain C++ hipcc does not add the HIP headers' directory itself).
ROCM_PATH ?= /opt/rocm
HOSTFLAGS = -O3 -std=c++17 -fPIC -Wall -Iasync_amd/csrc -Iinclude -isystem $(ROCM_PATH)/include
CFLAGS    = -O2 -std=c11 -fPIC -Wall -Wextra -Wno-unused-parameter -Iinclude

LIB      = async_amd/libasync_b64.so
# Stages + kernels only (no event loop/streams/allocator): the drop-in for a
# build of the reference library, which supplies async_wound(), the streams
# and (through fsdyn) fsalloc()/fsfree().
CORE     = async_amd/libasync_b64_core.so
ORACLE   = oracle/liboracle.so
HARNESS  = tests/csrc/libstage_harness.so
OBJDIR   = build

KERNEL_SRC = async_amd/csrc/b64x_kernels.hip
# Host resource management (placement, sessions, lanes), and what it shares
# with the kernel unit: the launchers it calls and the result check.
SESSIONS_SRC = async_amd/csrc/b64x_sessions.cpp
KERNEL_HDRS  = async_amd/csrc/b64x_launch.h async_amd/csrc/b64x_result_check.h
WRAP_SRC   = async_amd/csrc/b64x_wrap.hip
STRICT_SRC = async_amd/csrc/b64x_strict.hip
BATCH_SRC  = async_amd/csrc/b64x_lines_batch.hip
SKIP_SRC   = async_amd/csrc/b64x_skip.hip
ROWS_SRC   = async_amd/csrc/b64x_skip_rows.hip
PIECES_SRC = async_amd/csrc/b64x_skip_pieces.hip
WIDE_SRC   = async_amd/csrc/b64x_skip_wide.hip
PW_SRC     = async_amd/csrc/b64x_skip_pieces_wide.hip
EW_SRC     = async_amd/csrc/b64x_encode_wide.hip
SW_SRC     = async_amd/csrc/b64x_strict_wide.hip
# What the units of the strict decode that skips line breaks share, and the
# walk of its two one-pass units.
SKIP_HDRS  = async_amd/csrc/b64x_skip_body.h
WALK_HDRS  = async_amd/csrc/b64x_skip_walk.h
# The launch plan of the one-large-piece unit (no HIP in it).
WIDE_HDRS  = async_amd/csrc/b64x_skip_wide_plan.h
# The launch plan of the many-pieces-of-any-size unit (no HIP in it either).
PW_HDRS    = async_amd/csrc/b64x_skip_pieces_wide_plan.h $(WIDE_HDRS)
# The plan of the ragged encode balanced over bytes (no HIP in it either).
EW_HDRS    = async_amd/csrc/b64x_encode_wide_plan.h
# The plan of the ragged strict decode balanced over bytes (no HIP in it
# either; the shares' saturating arithmetic is the encode plan's).
SW_HDRS    = async_amd/csrc/b64x_strict_wide_plan.h $(EW_HDRS)
# Every header the line-wrapped encode, the strict decode and their ragged
# forms include: the plan arithmetic, the common device header and the
# per-lane bodies the one-buffer and the ragged-batch units share.
LINES_HDRS = async_amd/csrc/b64x_lines_plan.h async_amd/csrc/b64x_lines_dev.h \
             async_amd/csrc/b64x_wrap_body.h async_amd/csrc/b64x_strict_body.h
HOST_SRC   = async_amd/csrc/fsalloc.c async_amd/csrc/loop.c async_amd/csrc/streams.c \
             async_amd/csrc/framing.c async_amd/csrc/fdstreams.c async_amd/csrc/b64_hub.c \
             async_amd/csrc/b64_stages.c async_amd/csrc/b64_pin.c
HEADERS    = $(wildcard include/*.h)

HOST_OBJ   = $(patsubst async_amd/csrc/%.c,$(OBJDIR)/%.o,$(HOST_SRC))
# The GPU side of every library next to its kernel object (b64x_kernels.o, or
# the hooks build of it): the ten satellite code objects, in link order,
# and the host-only sessions unit.
GPU_OBJ    = $(OBJDIR)/b64x_wrap.o $(OBJDIR)/b64x_strict.o $(OBJDIR)/b64x_lines_batch.o \
             $(OBJDIR)/b64x_skip.o $(OBJDIR)/b64x_skip_rows.o $(OBJDIR)/b64x_skip_pieces.o \
             $(OBJDIR)/b64x_skip_wide.o $(OBJDIR)/b64x_skip_pieces_wide.o $(OBJDIR)/b64x_encode_wide.o \
             $(OBJDIR)/b64x_strict_wide.o $(OBJDIR)/b64x_sessions.o

# The same harness over the product's host C with a CPU stand-in for the GPU
# side (tests/csrc/fake_b64x.c): deterministic, adversarially ordered tests
# of the stages' slot accounting, no GPU needed (test infrastructure only).
FAKE     = tests/csrc/libstage_fake.so
# The kernels again with the test-only hooks compiled in (B64X_TEST_HOOKS:
# forced decode range lengths); never linked into the product libraries.
HOOKS    = tests/csrc/libb64x_hooks.so

all: $(LIB) $(CORE) $(ORACLE) $(HARNESS) $(FAKE) $(HOOKS)

$(OBJDIR):
	mkdir -p $(OBJDIR)

$(OBJDIR)/b64x_kernels.o: $(KERNEL_SRC) $(HEADERS) $(KERNEL_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# Thread placement, sessions and batch lanes: host code only, no device pass.
$(OBJDIR)/b64x_sessions.o: $(SESSIONS_SRC) $(HEADERS) $(KERNEL_HDRS) | $(OBJDIR)
	$(HIPCC) -x c++ -D__HIP_PLATFORM_AMD__ $(HOSTFLAGS) -c $< -o $@

# The line-wrapped encode: a code object of its own, linked after the kernels'.
$(OBJDIR)/b64x_wrap.o: $(WRAP_SRC) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# The strict decode: likewise, linked after both.
$(OBJDIR)/b64x_strict.o: $(STRICT_SRC) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# Their ragged-batch forms: likewise, linked after all three.
$(OBJDIR)/b64x_lines_batch.o: $(BATCH_SRC) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# The strict decode that skips line breaks: likewise, linked after all four.
$(OBJDIR)/b64x_skip.o: $(SKIP_SRC) $(SKIP_HDRS) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# Its one-pass form for strided rows: likewise, linked after all five.
$(OBJDIR)/b64x_skip_rows.o: $(ROWS_SRC) $(WALK_HDRS) $(SKIP_HDRS) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# The same walk over texts that arrive in pieces: likewise, linked after all six.
$(OBJDIR)/b64x_skip_pieces.o: $(PIECES_SRC) $(WALK_HDRS) $(SKIP_HDRS) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# One large piece, a wave per tile: likewise, linked after all seven.
$(OBJDIR)/b64x_skip_wide.o: $(WIDE_SRC) $(WIDE_HDRS) $(WALK_HDRS) $(SKIP_HDRS) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# Many pieces of any size, a wave per tile of each: likewise, linked after all eight.
$(OBJDIR)/b64x_skip_pieces_wide.o: $(PW_SRC) $(PW_HDRS) $(WALK_HDRS) $(SKIP_HDRS) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# The ragged encode balanced over bytes, plain and wrapped: likewise, linked after all nine.
$(OBJDIR)/b64x_encode_wide.o: $(EW_SRC) $(EW_HDRS) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# The ragged strict decode balanced over bytes, plain and wrapped: likewise, linked after all ten.
$(OBJDIR)/b64x_strict_wide.o: $(SW_SRC) $(SW_HDRS) $(LINES_HDRS) $(HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJDIR)/%.o: async_amd/csrc/%.c $(HEADERS) async_amd/csrc/b64_hub.h async_amd/csrc/b64_lend.h async_amd/csrc/b64_pin.h | $(OBJDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(OBJDIR)/b64x_kernels_hooks.o: $(KERNEL_SRC) $(HEADERS) $(KERNEL_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -DB64X_TEST_HOOKS -c $< -o $@

$(HOOKS): $(OBJDIR)/b64x_kernels_hooks.o $(GPU_OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^ -Wl,-soname,libb64x_hooks.so

$(LIB): $(OBJDIR)/b64x_kernels.o $(GPU_OBJ) $(HOST_OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^ -Wl,-soname,libasync_b64.so

$(CORE): $(OBJDIR)/b64x_kernels.o $(GPU_OBJ) $(OBJDIR)/b64_hub.o $(OBJDIR)/b64_stages.o $(OBJDIR)/b64_pin.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^ -Wl,-soname,libasync_b64_core.so

$(ORACLE): oracle/b64_oracle.c oracle/b64_oracle.h
	$(CC) -O2 -std=c11 -fPIC -Wall -Wextra -shared -o $@ oracle/b64_oracle.c

$(HARNESS): tests/csrc/stage_harness.c $(LIB) $(HEADERS)
	$(CC) $(CFLAGS) -shared -o $@ tests/csrc/stage_harness.c \
	    -Lasync_amd -lasync_b64 -Wl,-rpath,'$$ORIGIN/../../async_amd' \
	    -L/opt/rocm/lib -lamdhip64 -lpthread

$(FAKE): tests/csrc/stage_harness.c tests/csrc/fake_b64x.c oracle/b64_oracle.c $(HOST_SRC) $(HEADERS) \
         async_amd/csrc/b64_hub.h async_amd/csrc/b64_lend.h async_amd/csrc/b64x_result_check.h
	$(CC) $(CFLAGS) -Ioracle -Iasync_amd/csrc -shared -o $@ tests/csrc/stage_harness.c \
	    tests/csrc/fake_b64x.c oracle/b64_oracle.c $(HOST_SRC) -lpthread

clean:
	rm -rf $(OBJDIR) $(LIB) $(CORE) $(ORACLE) $(HARNESS) $(FAKE) $(HOOKS)

.PHONY: all clean

