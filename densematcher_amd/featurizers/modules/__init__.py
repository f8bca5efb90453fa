"""the building blocks of the aggregation network: resnet (BottleneckBlock, Conv2d, get_norm), projection_network (AggregationNetwork)"""
