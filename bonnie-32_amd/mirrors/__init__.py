"""The numpy / float32 restatements of the reference's editor rules (layout: the package docstring): no library, no binding, no GPU."""
