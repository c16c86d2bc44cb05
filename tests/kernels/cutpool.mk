# The kernel harness of the cut pool (test infrastructure): extern "C" entries that run relp::launch_cutpool_separate and
# relp::launch_cutpool_add_operands of the shipped librelp_engine.so on device images a test constructs
# (tests/kernel_harness_cutpool.py).
# `make -C tests/kernels -f cutpool.mk`
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc

all: librelp_kernel_harness_cutpool.so

librelp_kernel_harness_cutpool.so: harness_cutpool.cpp harness_pool_common.hpp $(CSRC)/relp_kernels.h $(CSRC)/relp_pool.hpp $(CSRC)/relp_layout.hpp $(ROOT)/rust-lp_amd/librelp_engine.so
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -Wall -Wextra -x hip -shared -I$(CSRC) -I$(ROOT)/include $< -o $@ \
	    -L$(ROOT)/rust-lp_amd -lrelp_engine -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd'

clean:
	rm -f librelp_kernel_harness_cutpool.so
