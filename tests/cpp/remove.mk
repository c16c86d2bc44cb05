# Cut rows and added columns removed in place.  `make -C tests/cpp -f remove.mk`
#   test_remove         through include/relp.hpp (remove_cuts, remove_columns, removal_stats, the refusals): pure C++17 against the C
#                       ABI, like test_tableau in the Makefile beside this file; runs on the GPU
#   test_layout_remove  Layout::remove_cuts / remove_columns (relp_layout.cpp is plain C++17): plain g++, no library, no GPU
CXX ?= g++
ROOT := ../..

all: test_remove test_layout_remove

test_remove: test_remove.cpp $(ROOT)/include/relp.hpp $(ROOT)/include/relp_engine.h $(ROOT)/rust-lp_amd/librelp_engine.so
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(ROOT)/rust-lp_amd -lrelp_engine \
	    -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd' -Wl,-rpath-link,/opt/rocm/lib

test_layout_remove: test_layout_remove.cpp $(ROOT)/rust-lp_amd/csrc/relp_layout.cpp $(ROOT)/rust-lp_amd/csrc/relp_layout.hpp $(ROOT)/include/relp_engine.h
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/rust-lp_amd/csrc test_layout_remove.cpp $(ROOT)/rust-lp_amd/csrc/relp_layout.cpp -o $@

clean:
	rm -f test_remove test_layout_remove
