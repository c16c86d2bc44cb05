# The kernel harness of the rows and columns removed in place (test infrastructure): one extern "C" entry that runs
# relp::launch_tab_compact of the shipped librelp_engine.so on a device image a test constructs (tests/kernel_harness_remove.py).
# `make -C tests/kernels -f remove.mk`
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc

all: librelp_kernel_harness_remove.so

librelp_kernel_harness_remove.so: harness_remove.cpp $(CSRC)/relp_kernels.h $(CSRC)/relp_layout.hpp $(ROOT)/rust-lp_amd/librelp_engine.so
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -Wall -Wextra -x hip -shared -I$(CSRC) -I$(ROOT)/include $< -o $@ \
	    -L$(ROOT)/rust-lp_amd -lrelp_engine -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd'

clean:
	rm -f librelp_kernel_harness_remove.so
