# The reference executor itself, compiled into oracle/_ref/ (test
# infrastructure, never committed, never linked by the product), and
# ref_driver, our own program over its public API (ref_driver.cpp).
#
# Nothing of the reference is kept here: its sources are found by globbing
# when make runs, and its config.hpp is generated from its own config.hpp.in.
# Where the reference tree is absent (a machine that received oracle/_ref/
# already built) every target below is a no-op that succeeds.
GINKGO_REF ?= /root/reference
REF_OUT := _ref
REF_CXX ?= g++
# -ffp-contract=off: no fused multiply-add the reference's source does not
# spell out; no -march=native, no fast-math: the bits must not depend on the
# build machine.
REF_CXXFLAGS := -std=c++14 -O1 -fPIC -ffp-contract=off -pthread -w
REF_INC := -I$(REF_OUT)/include -I$(GINKGO_REF)/include -I$(GINKGO_REF)
# MAX_JOBS if set, else 8 or the CPU count if smaller; never more than 16
REF_JOBS := $(shell j=$${MAX_JOBS:-8}; c=$$(nproc 2>/dev/null || echo 1); \
	[ -n "$${MAX_JOBS}" ] || { [ $$c -lt $$j ] && j=$$c; }; \
	[ $$j -gt 16 ] && j=16; [ $$j -lt 1 ] && j=1; echo $$j)

ifneq ($(wildcard $(GINKGO_REF)/include/ginkgo/config.hpp.in),)

REF_SRCS := $(shell cd $(GINKGO_REF) && find core reference devices -name '*.cpp' \
	! -path '*/test/*' ! -path 'core/mpi/*' ! -path '*/distributed/*' \
	! -path 'core/log/papi.cpp' \
	! -path 'core/device_hooks/reference_hooks.cpp' \
	! -path 'core/device_hooks/common_kernels.inc.cpp' | sort)
REF_OBJS := $(patsubst %.cpp,$(REF_OUT)/obj/%.o,$(REF_SRCS))
REF_CONFIG := $(REF_OUT)/include/ginkgo/config.hpp

# build() calls plain `make`; the parallelism is chosen here
ref:
	@$(MAKE) --no-print-directory -j$(REF_JOBS) $(REF_OUT)/ref_driver

# version 1.5.0, quiet, cxxabi.h present; no HIP platform, PAPI, MPI, HWLOC
$(REF_CONFIG): $(GINKGO_REF)/include/ginkgo/config.hpp.in
	@mkdir -p $(dir $@)
	sed -e 's/@Ginkgo_VERSION_MAJOR@/1/g' -e 's/@Ginkgo_VERSION_MINOR@/5/g' \
	    -e 's/@Ginkgo_VERSION_PATCH@/0/g' -e 's/@Ginkgo_VERSION_TAG@/master/g' \
	    -e 's/@GINKGO_VERBOSE_LEVEL@/0/g' \
	    -e 's/^#cmakedefine GKO_HAVE_CXXABI_H/#define GKO_HAVE_CXXABI_H/' \
	    -e 's/@GINKGO_HIP_PLATFORM_HCC@/0/g' -e 's/@GINKGO_HIP_PLATFORM_NVCC@/0/g' \
	    -e 's/@GINKGO_HAVE_PAPI_SDE@/0/g' -e 's/@GINKGO_HAVE_HWLOC@/0/g' \
	    -e 's/^#cmakedefine01 \([A-Z_]*\)/#define \1 0/' \
	    -e 's/^#cmakedefine \([A-Z_]*\)/\/* #undef \1 *\//' $< > $@.tmp
	mv $@.tmp $@

$(REF_OUT)/obj/%.o: $(GINKGO_REF)/%.cpp $(REF_CONFIG)
	@mkdir -p $(dir $@)
	$(REF_CXX) $(REF_CXXFLAGS) $(REF_INC) -MMD -MP -c $< -o $@

$(REF_OUT)/ref_driver.o: ref_driver.cpp $(REF_CONFIG)
	@mkdir -p $(dir $@)
	$(REF_CXX) $(REF_CXXFLAGS) $(REF_INC) -MMD -MP -c $< -o $@

# the C++ runtime goes in statically: the driver also runs on machines that
# have only libc, libm and libpthread
$(REF_OUT)/ref_driver: $(REF_OUT)/ref_driver.o $(REF_OBJS)
	$(REF_CXX) -pthread -static-libstdc++ -static-libgcc -s -o $@.tmp $^ -lm
	mv $@.tmp $@

ref-objs: $(REF_OBJS)

-include $(REF_OUT)/ref_driver.d $(REF_OBJS:.o=.d)

else

ref:
	@true

endif

ref-where:
	@echo $(GINKGO_REF)

ref-clean:
	rm -rf $(REF_OUT)
.PHONY: ref ref-objs ref-where ref-clean
