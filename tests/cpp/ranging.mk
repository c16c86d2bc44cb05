# The batched ratio queries through include/relp.hpp (row_ratios, rhs_ranging, ranging_stats): pure C++17 against the C ABI, like
# test_tableau in the Makefile beside this file.  `make -C tests/cpp -f ranging.mk`
CXX ?= g++
ROOT := ../..

all: test_ranging

test_ranging: test_ranging.cpp $(ROOT)/include/relp.hpp $(ROOT)/include/relp_engine.h $(ROOT)/rust-lp_amd/librelp_engine.so
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(ROOT)/rust-lp_amd -lrelp_engine \
	    -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd' -Wl,-rpath-link,/opt/rocm/lib

clean:
	rm -f test_ranging
