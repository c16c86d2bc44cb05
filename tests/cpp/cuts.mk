# Cut rows added in place.  `make -C tests/cpp -f cuts.mk`
#   test_cuts         through include/relp.hpp (add_cuts, reserve_cuts, run_dual, objective): pure C++17 against the C ABI, like
#                     test_tableau in the Makefile beside this file; runs on the GPU
#   test_layout_cuts  Layout::add_cuts (relp_layout.cpp is plain C++17): plain g++, no library, no GPU
CXX ?= g++
ROOT := ../..

all: test_cuts test_layout_cuts

test_cuts: test_cuts.cpp $(ROOT)/include/relp.hpp $(ROOT)/include/relp_engine.h $(ROOT)/rust-lp_amd/librelp_engine.so
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(ROOT)/rust-lp_amd -lrelp_engine \
	    -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd' -Wl,-rpath-link,/opt/rocm/lib

test_layout_cuts: test_layout_cuts.cpp $(ROOT)/rust-lp_amd/csrc/relp_layout.cpp $(ROOT)/rust-lp_amd/csrc/relp_layout.hpp $(ROOT)/include/relp_engine.h
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/rust-lp_amd/csrc test_layout_cuts.cpp $(ROOT)/rust-lp_amd/csrc/relp_layout.cpp -o $@

clean:
	rm -f test_cuts test_layout_cuts
