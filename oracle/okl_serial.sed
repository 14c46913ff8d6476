# okl_serial.sed -- OKL kernel file -> C++ with OCCA-Serial semantics.
#
# Holds for kernel files whose only annotations are @kernel, @tile(.., @outer,
# @inner), @outer, @inner and @shared: without @barrier and @exclusive every
# @inner loop runs to its end before the next statement, so Serial mode is the
# plain loop nest and @shared arrays are per-@outer scratch.  oracle/Makefile
# refuses the result if any '@' is left, so a kernel file that needs more than
# these four rewrites stops the build instead of being mistranslated.
s/@kernel/extern "C"/g
s/; *@tile([^()]*))/)/g
s/; *@outer)/)/g
s/; *@inner)/)/g
s/@shared //g
