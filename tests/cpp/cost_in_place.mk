# The in-place cost change through include/relp.hpp (change_cost, set_cost, run, objective): pure C++17 against the C ABI, like
# test_tableau in the Makefile beside this file.  `make -C tests/cpp -f cost_in_place.mk`
CXX ?= g++
ROOT := ../..

all: test_cost_in_place

test_cost_in_place: test_cost_in_place.cpp $(ROOT)/include/relp.hpp $(ROOT)/include/relp_engine.h $(ROOT)/rust-lp_amd/librelp_engine.so
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(ROOT)/rust-lp_amd -lrelp_engine \
	    -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd' -Wl,-rpath-link,/opt/rocm/lib

clean:
	rm -f test_cost_in_place
