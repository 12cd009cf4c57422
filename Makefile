# Plain-make build of the product for C/C++ users (python -m libsrcnn_amd.build does the same).
#   make            -> libsrcnn_amd/lib/libsrcnn_amd.so + libsrcnn.so + libsrcnn.a + libsrcnn_amd/bin/srcnntest + srcnnyuv
#                      libsrcnn.so / libsrcnn.a: the names the reference's Makefiles produce (Makefiles/Makefile.linux:13-14,
#                      38-39) -- a program linked with -lsrcnn runs on this library without relinking
#   make install    -> $(DESTDIR)$(PREFIX)/lib/{libsrcnn_amd.so,libsrcnn.so,libsrcnn.a}, include/{libsrcnn.h,srcnn_amd.h}
#                      (the reference's install / uninstall: Makefiles/Makefile.linux:64-75)
#   make install-yuv -> the same + include/srcnn_amd_yuv.h, srcnn_amd_yuv_ex.h, srcnn_amd_yuv_packed.h (the YUV extensions)
#   make install-rgb -> the same as install + include/srcnn_amd_rgb.h (RGB(A) images in device memory)
#   make install-rect -> the same as install + include/srcnn_amd_rect.h (one rectangle of the Y path's output)
#                      and include/srcnn_amd_rect_list.h (a list of them in one call) and include/srcnn_amd_delta.h (only what
#                      changed between two frames)
#   make install-yuv-packed-rect -> the same as install-yuv and install-rect + include/srcnn_amd_yuv_packed_rect.h (one rectangle of
#                      a packed frame) and include/srcnn_amd_yuv_packed_rect_list.h (a list of them in one call)
#   make oracle     -> the CPU checker (and oracle/_ref where the reference tree is present)
#   make test       -> CPU test-suite;  make gpu-test on a gfx950 box
#   make ubench     -> tools/ubench/bin/* (microbenchmarks; hipcc, gfx950)
#   make asan tsan  -> the host code (table builder, drop-in control flow, frame-call argument checks, owner types, oracle) under ASan+UBSan / TSan, CPU only
#   make pipeline-asan pipeline-tsan -> the threaded host pipeline (srcnn_capi.cpp, srcnn_pipeline.cpp: lanes, bands, bounce slots, async jobs,
#                      frame stream and graphs, several contexts) on a fake HIP runtime under the same sanitizers, CPU only
#   make STRICT_ONLY=1 -> the same artefacts under libsrcnn_amd/lib/strict/ with NO non-parity kernel compiled in (no FAST /
#                      FAST_F16 / RELAXED template instance, no srcnn_fused_f16.hip); srcnn_set_mode refuses those modes
HIPCC   ?= /opt/rocm/bin/hipcc
CSRC    := libsrcnn_amd/csrc
ifeq ($(STRICT_ONLY),1)
LIBDIR  := libsrcnn_amd/lib/strict
BINDIR  := libsrcnn_amd/lib/strict/bin
STRICT_DEF := -DSRCNN_STRICT_ONLY
else
LIBDIR  := libsrcnn_amd/lib
BINDIR  := libsrcnn_amd/bin
STRICT_DEF :=
endif
# -ffp-contract=off: the strict kernels and the host table builder must round every multiply and add separately
HIPFLAGS := --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -fvisibility=hidden -Wall \
            -Wno-unused-result -Wno-unused-value -Wno-ignored-attributes -D__HIP_PLATFORM_AMD__ $(STRICT_DEF)
ifeq ($(STRICT_ONLY),1)
SRCS    := srcnn_kernels.hip srcnn_yuv_planes.hip srcnn_yuv_packed.hip srcnn_rgb.hip srcnn_rgb_window.hip srcnn_yuv_window.hip srcnn_yuv_packed_window.hip srcnn_window.hip srcnn_rect_list.hip srcnn_rgb_rect_list.hip srcnn_yuv_rect_list.hip srcnn_yuv_packed_rect_list.hip srcnn_delta.hip srcnn_rect_list_call.cpp srcnn_rgb_rect_list_call.cpp srcnn_yuv_rect_list_call.cpp srcnn_yuv_packed_rect_list_call.cpp srcnn_delta_call.cpp srcnn_rgb_delta_call.cpp srcnn_capi.cpp srcnn_frames.cpp srcnn_pipeline.cpp srcnn_comm.cpp dropin.cpp
else
SRCS    := srcnn_kernels.hip srcnn_fused_f16.hip srcnn_yuv_planes.hip srcnn_yuv_packed.hip srcnn_rgb.hip srcnn_rgb_window.hip srcnn_yuv_window.hip srcnn_yuv_packed_window.hip srcnn_window.hip srcnn_rect_list.hip srcnn_rgb_rect_list.hip srcnn_yuv_rect_list.hip srcnn_yuv_packed_rect_list.hip srcnn_delta.hip srcnn_rect_list_call.cpp srcnn_rgb_rect_list_call.cpp srcnn_yuv_rect_list_call.cpp srcnn_yuv_packed_rect_list_call.cpp srcnn_delta_call.cpp srcnn_rgb_delta_call.cpp srcnn_capi.cpp srcnn_frames.cpp srcnn_pipeline.cpp srcnn_comm.cpp dropin.cpp
endif
OBJS    := $(addprefix $(LIBDIR)/,$(addsuffix .o,$(basename $(SRCS))))
HDRS    := $(CSRC)/srcnn_kernels.h $(CSRC)/srcnn_yuv.h $(CSRC)/srcnn_rgb.h $(CSRC)/srcnn_window.h $(CSRC)/srcnn_frame_rules.h $(CSRC)/srcnn_frame_args.hpp $(CSRC)/srcnn_rect_source.hpp $(CSRC)/srcnn_y_path_geom.hpp $(CSRC)/srcnn_rect_atlas.hpp $(CSRC)/srcnn_rgb_rect_atlas.hpp $(CSRC)/srcnn_yuv_rect_atlas.hpp $(CSRC)/srcnn_yuv_packed_rect_atlas.hpp $(CSRC)/srcnn_yuv_chroma_tile.h $(CSRC)/srcnn_yuv_packed_merge_tile.h $(CSRC)/srcnn_rect_list.h $(CSRC)/srcnn_rect_list_call.hpp $(CSRC)/srcnn_delta.h $(CSRC)/srcnn_delta.hpp $(CSRC)/srcnn_delta_call.hpp $(CSRC)/srcnn_rgb_delta.hpp $(CSRC)/srcnn_pixel_io.h $(CSRC)/srcnn_colour_rules.h $(CSRC)/srcnn_window_tile.h $(CSRC)/srcnn_yuv_packed_fields.h $(CSRC)/srcnn_host.hpp $(CSRC)/srcnn_owned.hpp $(CSRC)/srcnn_settings.hpp $(CSRC)/srcnn_watchdog.hpp $(CSRC)/resample_table.hpp $(CSRC)/srcnn_weights.inc include/srcnn_amd.h include/srcnn_amd_debug.h include/srcnn_amd_yuv.h include/srcnn_amd_yuv_ex.h include/srcnn_amd_yuv_packed.h include/srcnn_amd_rgb.h include/srcnn_amd_rect.h include/srcnn_amd_rect_list.h include/srcnn_amd_rgb_rect.h include/srcnn_amd_rgb_rect_list.h include/srcnn_amd_yuv_rect.h include/srcnn_amd_yuv_rect_list.h include/srcnn_amd_yuv_packed_rect.h include/srcnn_amd_yuv_packed_rect_list.h include/srcnn_amd_delta.h include/srcnn_amd_rgb_delta.h include/libsrcnn_dropin.h

PREFIX  ?= /usr/local
ROCM    ?= /opt/rocm

all: $(LIBDIR)/libsrcnn_amd.so $(LIBDIR)/libsrcnn.so $(LIBDIR)/libsrcnn.a $(BINDIR)/srcnntest $(BINDIR)/srcnnyuv

$(LIBDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_$*) -x hip -c $< -o $@
# the fused kernel is issue-bound beside its MFMAs, where packed fp32 VALU ops are an anti-lever: no SLP packing there
EXTRA_srcnn_fused_f16 := -fno-slp-vectorize

$(LIBDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

# exports.map: only srcnn_* and the two reference symbols are exported (the kernels' launch stubs are not)
$(LIBDIR)/libsrcnn_amd.so: $(OBJS) $(CSRC)/exports.map
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC $(OBJS) -o $@ -ldl -Wl,-soname,libsrcnn_amd.so -Wl,--version-script=$(CSRC)/exports.map

# libsrcnn.so: what a program linked against the reference's shared library asks the loader for (the reference links it
# without a soname, so the request is the file name): a symbolic link to the product.  New links with -lsrcnn record the
# product's soname (libsrcnn_amd.so), old binaries find the file they ask for.
$(LIBDIR)/libsrcnn.so: $(LIBDIR)/libsrcnn_amd.so
	ln -sf libsrcnn_amd.so $@

# libsrcnn.a: the reference's DEFAULT artefact is the static library.  Consumers add the HIP runtime to their link line:
#   g++ app.o -L<libdir> -lsrcnn -L$(ROCM)/lib -lamdhip64 -ldl -lpthread      (instead of the reference's -lsrcnn -fopenmp)
$(LIBDIR)/libsrcnn.a: $(OBJS)
	rm -f $@ && ar crs $@ $(OBJS)

$(BINDIR)/srcnntest: tools/srcnntest.cpp $(LIBDIR)/libsrcnn_amd.so
	@mkdir -p $(BINDIR)
	g++ -O2 -std=c++17 $< -L$(LIBDIR) -lsrcnn_amd -Wl,-rpath,$(abspath $(LIBDIR)) -Wl,-rpath,'$$ORIGIN/../lib' -o $@

# YUV4MPEG2 streams through srcnn_yuv420_upscale_dev / srcnn_yuv_upscale_dev (include/srcnn_amd_yuv.h, srcnn_amd_yuv_ex.h)
$(BINDIR)/srcnnyuv: tools/srcnnyuv.cpp include/srcnn_amd_yuv.h include/srcnn_amd_yuv_ex.h $(LIBDIR)/libsrcnn_amd.so
	@mkdir -p $(BINDIR)
	g++ -O2 -std=c++17 $< -L$(LIBDIR) -lsrcnn_amd -Wl,-rpath,$(abspath $(LIBDIR)) -Wl,-rpath,'$$ORIGIN/../lib' -o $@

# the microbenchmarks behind profiles/r0x_*.txt (outputs are NOT tracked: tools/ubench/bin/ is git-ignored)
UBENCH_HIP := $(wildcard tools/ubench/*.hip) $(wildcard tools/ubench/*.cpp)
ubench: $(patsubst tools/ubench/%,tools/ubench/bin/%,$(basename $(UBENCH_HIP)))
tools/ubench/bin/%: tools/ubench/%.hip
	@mkdir -p tools/ubench/bin
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 $< -o $@
tools/ubench/bin/%: tools/ubench/%.cpp
	@mkdir -p tools/ubench/bin
	$(HIPCC) --offload-arch=gfx950 -O2 -std=c++17 -x hip $< -o $@ -lpthread

oracle:
	$(MAKE) -C oracle all
	@if [ -d /root/reference/src ]; then $(MAKE) -C oracle ref; fi

test: all oracle
	python -m pytest tests -x -q -m "not gpu"

gpu-test: all oracle
	python -m pytest tests -x -q -m gpu

# CPU-only sanitizer builds of the host code (no GPU sanitizer exists on this pool): tests/host/host_sanitize.cpp
SAN_SRCS := tests/host/host_sanitize.cpp $(CSRC)/dropin.cpp
SAN_DEPS := $(SAN_SRCS) $(CSRC)/resample_table.hpp $(CSRC)/srcnn_watchdog.hpp $(CSRC)/srcnn_frame_args.hpp $(CSRC)/srcnn_y_path_geom.hpp $(CSRC)/srcnn_frame_rules.h $(CSRC)/srcnn_owned.hpp oracle/srcnn_oracle.c include/srcnn_amd.h include/srcnn_amd_debug.h include/srcnn_amd_yuv.h include/srcnn_amd_yuv_ex.h include/srcnn_amd_yuv_packed.h include/srcnn_amd_rgb.h include/libsrcnn_dropin.h
tests/host/_build/oracle_%.o: oracle/srcnn_oracle.c oracle/oracle_weights.inc
	@mkdir -p tests/host/_build
	gcc -O1 -g -ffp-contract=off -std=c99 -fsanitize=$(subst asan,address$(comma)undefined,$(subst tsan,thread,$*)) -fno-omit-frame-pointer -c $< -o $@
comma := ,
tests/host/_build/host_asan: $(SAN_DEPS) tests/host/_build/oracle_asan.o
	g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
	    $(SAN_SRCS) tests/host/_build/oracle_asan.o -lm -o $@
tests/host/_build/host_tsan: $(SAN_DEPS) tests/host/_build/oracle_tsan.o
	g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=thread -fno-omit-frame-pointer \
	    $(SAN_SRCS) tests/host/_build/oracle_tsan.o -lm -lpthread -o $@
asan: tests/host/_build/host_asan
	ASAN_OPTIONS=detect_leaks=1:alloc_dealloc_mismatch=1:strict_string_checks=1 UBSAN_OPTIONS=print_stacktrace=1 $<
tsan: tests/host/_build/host_tsan
	TSAN_OPTIONS=halt_on_error=1 $<

# The threaded host pipeline itself (srcnn_capi.cpp, srcnn_pipeline.cpp, srcnn_comm.cpp, dropin.cpp, unchanged) on a fake HIP
# runtime and CPU launchers: tests/host/pipeline_sanitize.cpp.  Plain C++ with the ROCm clang (g++ has no _Float16 here).
PIPE_CXX  := $(ROCM)/lib/llvm/bin/clang++
PIPE_SRCS := tests/host/pipeline_sanitize.cpp tests/host/fake_hip.cpp tests/host/fake_kernels.cpp $(CSRC)/srcnn_capi.cpp $(CSRC)/srcnn_pipeline.cpp $(CSRC)/srcnn_comm.cpp $(CSRC)/dropin.cpp
PIPE_FLAGS := -O1 -g -std=c++17 -ffp-contract=off -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Wno-unused-value -Wno-unused-result
PIPE_SAN_asan := -fsanitize=address,undefined -fno-sanitize-recover=undefined
PIPE_SAN_tsan := -fsanitize=thread
# the oracle is the single-threaded reference of the comparison: ASan and UBSan check it, TSan has nothing to see in it and
# would only slow it down (it is a third of the harness's arithmetic)
PIPE_ORACLE_SAN_asan := $(PIPE_SAN_asan)
PIPE_ORACLE_SAN_tsan :=
PIPE_UNITS := pipeline_sanitize fake_hip fake_kernels srcnn_capi srcnn_pipeline srcnn_comm dropin oracle
PIPE_DEPS := $(PIPE_SRCS) $(HDRS) oracle/srcnn_oracle.c oracle/oracle_weights.inc
define pipe_rules
tests/host/_build/pipe_$(1)_%.o: tests/host/%.cpp $$(PIPE_DEPS)
	@mkdir -p tests/host/_build
	$$(PIPE_CXX) -x c++ $$(PIPE_FLAGS) $$(PIPE_SAN_$(1)) -c $$< -o $$@
tests/host/_build/pipe_$(1)_%.o: $$(CSRC)/%.cpp $$(PIPE_DEPS)
	@mkdir -p tests/host/_build
	$$(PIPE_CXX) -x c++ $$(PIPE_FLAGS) $$(PIPE_SAN_$(1)) -c $$< -o $$@
tests/host/_build/pipe_$(1)_oracle.o: oracle/srcnn_oracle.c oracle/oracle_weights.inc
	@mkdir -p tests/host/_build
	$$(PIPE_CXX) -x c -std=c99 -O1 -g -ffp-contract=off -fno-omit-frame-pointer $$(PIPE_ORACLE_SAN_$(1)) -c $$< -o $$@
# (the objects are built by a sub-make of their own, 8 at a time, whatever -j this make was given: at most 16 here)
tests/host/_build/pipeline_$(1): $$(PIPE_DEPS)
	@mkdir -p tests/host/_build
	@echo 'int main() { return 0; }' | $$(PIPE_CXX) -x c++ $$(PIPE_SAN_$(1)) - -o tests/host/_build/pipe_$(1)_probe 2>/dev/null || \
	    { echo "libpipeline-$(1): $$(PIPE_CXX) or its sanitizer runtime: No such file (tests/test_host_sanitizers.py skips on this line)" >&2; exit 1; }
	+$$(MAKE) -j8 $$(foreach u,$$(PIPE_UNITS),tests/host/_build/pipe_$(1)_$$(u).o)
	$$(PIPE_CXX) $$(PIPE_SAN_$(1)) $$(foreach u,$$(PIPE_UNITS),tests/host/_build/pipe_$(1)_$$(u).o) -lm -ldl -lpthread -o $$@
endef
$(eval $(call pipe_rules,asan))
$(eval $(call pipe_rules,tsan))
# every scenario as a process of its own (the library reads its switches once, at load), under both schedules of the fake
# runtime (the two run side by side: at most ten busy threads); the goal stops at the first scenario that fails
define pipe_run
	@set -e; for sc in `$(1) --list`; do \
	    env `$(1) --env $$sc` FAKE_HIP_SCHEDULE=asap $(2) $(1) $$sc & a=$$!; \
	    env `$(1) --env $$sc` FAKE_HIP_SCHEDULE=lazy $(2) $(1) $$sc & l=$$!; \
	    ra=0; rl=0; wait $$a || ra=$$?; wait $$l || rl=$$?; \
	    if [ $$ra != 0 ] || [ $$rl != 0 ]; then echo "pipeline scenario $$sc FAILED (asap: $$ra, lazy: $$rl)" >&2; exit 1; fi; \
	done
endef
pipeline-asan: tests/host/_build/pipeline_asan
	$(call pipe_run,$<,ASAN_OPTIONS=detect_leaks=1:alloc_dealloc_mismatch=1:strict_string_checks=1 UBSAN_OPTIONS=print_stacktrace=1)
	@echo "pipeline-asan: all checks passed"
pipeline-tsan: tests/host/_build/pipeline_tsan
	$(call pipe_run,$<,TSAN_OPTIONS=halt_on_error=1)
	@echo "pipeline-tsan: all checks passed"

install: all
	install -d $(DESTDIR)$(PREFIX)/lib $(DESTDIR)$(PREFIX)/include
	install -m 755 $(LIBDIR)/libsrcnn_amd.so $(DESTDIR)$(PREFIX)/lib/
	ln -sf libsrcnn_amd.so $(DESTDIR)$(PREFIX)/lib/libsrcnn.so
	install -m 644 $(LIBDIR)/libsrcnn.a $(DESTDIR)$(PREFIX)/lib/
	install -m 644 include/libsrcnn_dropin.h $(DESTDIR)$(PREFIX)/include/libsrcnn.h
	install -m 644 include/srcnn_amd.h $(DESTDIR)$(PREFIX)/include/srcnn_amd.h
	@if [ -z "$(DESTDIR)" ] && [ "$$(id -u)" = 0 ]; then ldconfig; fi

# the YUV extension headers (include/srcnn_amd_yuv.h, include/srcnn_amd_yuv_ex.h, include/srcnn_amd_yuv_packed.h) beside the stable one; `install` keeps the layout of the
# reference's install target
install-yuv: install
	install -m 644 include/srcnn_amd_yuv.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv.h
	install -m 644 include/srcnn_amd_yuv_ex.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv_ex.h
	install -m 644 include/srcnn_amd_yuv_packed.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv_packed.h

# the device-resident RGB(A) extension header (include/srcnn_amd_rgb.h)
install-rgb: install
	install -m 644 include/srcnn_amd_rgb.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_rgb.h

# the rect extension headers (include/srcnn_amd_rect.h, include/srcnn_amd_rect_list.h, include/srcnn_amd_delta.h)
install-rect: install
	install -m 644 include/srcnn_amd_rect.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_rect.h
	install -m 644 include/srcnn_amd_rect_list.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_rect_list.h
	install -m 644 include/srcnn_amd_delta.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_delta.h

# the packed rect extension headers: include/srcnn_amd_yuv_packed_rect.h, which includes srcnn_amd_yuv_packed.h, and
# include/srcnn_amd_yuv_packed_rect_list.h, which includes that one and srcnn_amd_rect_list.h
install-yuv-packed-rect: install-yuv install-rect
	install -m 644 include/srcnn_amd_yuv_packed_rect.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv_packed_rect.h
	install -m 644 include/srcnn_amd_yuv_packed_rect_list.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv_packed_rect_list.h

uninstall:
	rm -f $(DESTDIR)$(PREFIX)/lib/libsrcnn_amd.so $(DESTDIR)$(PREFIX)/lib/libsrcnn.so $(DESTDIR)$(PREFIX)/lib/libsrcnn.a
	rm -f $(DESTDIR)$(PREFIX)/include/libsrcnn.h $(DESTDIR)$(PREFIX)/include/srcnn_amd.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv_ex.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv_packed.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_rgb.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_rect.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_rect_list.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_delta.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv_packed_rect.h $(DESTDIR)$(PREFIX)/include/srcnn_amd_yuv_packed_rect_list.h
	@if [ -z "$(DESTDIR)" ] && [ "$$(id -u)" = 0 ]; then ldconfig; fi

clean:
	rm -rf $(LIBDIR) $(BINDIR) oracle/_build oracle/_ref tests/host/_build tools/ubench/bin

.PHONY: all oracle test gpu-test clean asan tsan pipeline-asan pipeline-tsan ubench install install-yuv install-rgb install-rect install-yuv-packed-rect uninstall
